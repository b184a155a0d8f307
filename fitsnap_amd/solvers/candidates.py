"""Batched candidate fits of a weight search (the genetic algorithm of examples/library/genetic_algorithm/libmod_optimize.py:
``update_weights`` + ``fit_and_cost``, one ``perform_fit`` and one ``error_analysis`` per candidate).

In that search every row's weight depends only on its (group, row type): a candidate scales the base weight ``w0`` of the
rows of category c = (group, testing, row type) -- the categories of ``Solver.error_analysis`` -- by ``S[p, c]``.  Then

    G_p = sum_c S[p, c]^2 G_c,   c_p = sum_c S[p, c]^2 r_c       (G_c, r_c: statistics of the training rows of c with w0)

so the rows are read once for the per-category statistics (``fsnap_cat_normal_eq``), a candidate costs a combination and
a K x K solve (``fsnap_fit_candidates``), and the residual sums of the error tables -- sum|r|, sum r^2, sum|w0 r|,
sum (w0 r)^2 per category -- come from one pass over the rows for up to 16 coefficient vectors (``fsnap_candidate_rows``).
The candidate-independent parts of the tables (counts, sums of the truths, their centred sums) are computed once.
"""
from __future__ import annotations

import numpy as np

from .. import _capi
from .solver import RCOND_MARGIN, Solver, _is_label_container, refinement_done, refinement_skip

ROW_TYPE_WEIGHT = {"Energy": "eweight", "Force": "fweight", "Stress": "vweight"}


def check_scales(S, ncat):
    """(P, ncat) float64 array of candidate scales, or ValueError."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim != 2 or S.shape[1] != ncat:
        raise ValueError(f"S must have shape (P, {ncat}) (one scale per candidate and category), got {S.shape}")
    if S.shape[0] == 0:
        raise ValueError("S holds no candidate (P = 0)")
    if not np.isfinite(S).all():
        raise ValueError("S holds non-finite scales")
    return np.ascontiguousarray(S)


def category_constants(t, w0, cat, ncat):
    """The candidate-independent columns of the ten sums of ``fsnap_error_stats`` per category, for the base weights:
    (ncat, 6) = n, count_nonzero(w0), sum t, sum w0 t, sum (t - mean t)^2, sum (w0 t - sum(w0 t) / n_w)^2."""
    t = np.asarray(t, dtype=np.float64)
    w0 = np.asarray(w0, dtype=np.float64)
    cat = np.asarray(cat, dtype=np.int64)
    keep = cat >= 0
    t, w0, cat = t[keep], w0[keep], cat[keep]

    def per_cat(x):
        return np.bincount(cat, weights=x, minlength=ncat)

    n = np.bincount(cat, minlength=ncat).astype(np.float64)
    nw = per_cat((w0 != 0).astype(np.float64))
    st, swt = per_cat(t), per_cat(w0 * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_t = np.where(n > 0, st / n, 0.0)
        mean_wt = np.where(nw > 0, swt / nw, 0.0)
    return np.stack([n, nw, st, swt, per_cat((t - mean_t[cat]) ** 2), per_cat((w0 * t - mean_wt[cat]) ** 2)], axis=1)


def assemble_sums(const, sums4, s):
    """(ncat, 10) sums of ``fsnap_error_stats`` for the weights w0 * s[c] from the constants of ``category_constants``
    and the four residual sums (sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2) of one candidate: the weighted columns scale
    with |s| or s^2, and a category with s = 0 has no row of non-zero weight."""
    const = np.asarray(const, dtype=np.float64).reshape(-1, 6)
    sums4 = np.asarray(sums4, dtype=np.float64).reshape(-1, 4)
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    a, s2 = np.abs(s), s * s
    return np.stack([const[:, 0], np.where(s != 0, const[:, 1], 0.0), const[:, 2], s * const[:, 3], sums4[:, 0], sums4[:, 1],
                     const[:, 4], a * sums4[:, 2], s2 * sums4[:, 3], s2 * const[:, 5]], axis=1)


class CandidateFits:
    """Fits and error tables of many weight candidates of one solver on the same rows.

    ``CandidateFits(solver, a=None, b=None, w0=None, fs_dict=None)``: the rows ``a``, ``b`` and the labels ``fs_dict``
    (``Groups``, ``Testing``, ``Row_Type``) default to the shared arrays and ``pt.fitsnap_dict`` as in ``perform_fit``;
    ``w0`` (one weight per row, default ones) is the base weight every candidate scales.  ``keys`` lists the categories
    (group, testing, row type) in the order of ``error_analysis``.

    ``fit(S)`` returns the (P, K) coefficients of P candidates, S[p, c] = scale of category c; every candidate takes the
    decisions ``perform_fit`` takes for the weights ``w0 * S[p, category]`` (probe solve, ``_resolve_probe``,
    refinement, row-space fallback), recorded in ``info``.  ``errors(betas, S)`` gives the tables of ``error_analysis``
    for the same weights; the bzeroflag offset is NOT applied: to write a candidate's potential, set
    ``solver.fit = betas[p].copy()``, call ``solver._offset()`` if the SNAP calculator has ``bzeroflag``, then
    ``write_output``.

    Supported: ``SVD`` and ``RIDGE`` (both ``local_solver`` settings).  Collective in a multi-rank job: every rank gets
    all coefficients; the error tables are pooled on rank 0 (other ranks get ``None``), as ``error_analysis`` does."""

    def __init__(self, solver, a=None, b=None, w0=None, fs_dict=None):
        from .ridge import RIDGE
        from .svd import SVD

        if not isinstance(solver, Solver):
            raise TypeError("CandidateFits needs a Solver instance")
        if not isinstance(solver, (SVD, RIDGE)):
            raise NotImplementedError(
                f"CandidateFits supports SVD and RIDGE: {type(solver).__name__} is not a linear solve of the per-category "
                "statistics (iterative, sampling or likelihood solvers need the rows for every candidate)")
        sections = solver.config.sections
        if "EXTRAS" in sections and sections["EXTRAS"].apply_transpose:
            raise NotImplementedError("CandidateFits does not support [EXTRAS] apply_transpose: the transpose trick solves "
                                      "G^T G instead of G, which is not a per-category sum of the statistics")
        self.solver = solver
        pt = solver.pt
        self.pt = pt
        self._shared = a is None and b is None
        if self._shared:
            a, b = pt.shared_arrays["a"].array, pt.shared_arrays["b"].array
        if fs_dict is None:
            local = getattr(pt, "local_lists", None)
            fs_dict = local if (pt.multi and local) else pt.fitsnap_dict
        a = np.asarray(a)
        b = np.asarray(b, dtype=np.float64)
        if a.ndim != 2 or b.shape != (a.shape[0],):
            raise ValueError("a must be (m, K) and b (m,)")
        m, K = a.shape
        self.a, self.b, self.K, self.m = a, b, K, m
        self.w0 = np.ones(m) if w0 is None else np.ascontiguousarray(w0, dtype=np.float64)
        if self.w0.shape != (m,):
            raise ValueError(f"w0 must have one weight per row ({m}), got shape {self.w0.shape}")
        self.fs_dict = fs_dict
        self.testing = np.asarray(fs_dict["Testing"], dtype=bool)
        if self.testing.shape != (m,):
            raise ValueError("fs_dict['Testing'] must have one entry per row")
        cat, keys = self._categories(fs_dict, m)
        if pt.multi:
            gkeys = solver._global_keys(keys)
            pos = {k: i for i, k in enumerate(gkeys)}
            remap = np.array([pos[k] for k in keys], dtype=np.int32)
            cat = np.where(cat >= 0, remap[np.maximum(cat, 0)], -1).astype(np.int32)
            keys = gkeys
        self.cat = cat
        self.keys = keys
        self.ncat = len(keys)
        self.const = category_constants(b, self.w0, cat, self.ncat)
        self.info = []
        self._layout = None          # tag of this object's category layout on the context (fsnap_cat_prepare)
        self._packed = None          # (context, device address, K, P) of the last fit's packed candidate statistics
        self._cv = None              # (tag, composite categories, F, device address of the blocks) of cross_validate's layout
        self._cv_folds = None        # (key, composite categories, fold_of_unit, F, rows per composite category) of its last folds

    @staticmethod
    def _categories(fs_dict, m):
        from pandas import DataFrame

        lists = (fs_dict["Groups"], fs_dict["Testing"], fs_dict["Row_Type"])
        if not all(_is_label_container(l) and len(l) == m for l in lists):
            raise ValueError("fs_dict needs Groups, Testing and Row_Type with one entry per row")
        gb = DataFrame({"Groups": lists[0], "Testing": lists[1], "Row_Type": lists[2]}).groupby(
            ["Groups", "Testing", "Row_Type"], sort=True, observed=True)
        return gb.ngroup().to_numpy(dtype=np.int32), list(gb.size().index)

    # ------------------------------------------------------------------------------
    def scales_from_group_weights(self, cands):
        """(P, ncat) scales from GA-style candidates ``[{group: {"eweight", "fweight", "vweight"}}]``, mapped as
        ``update_weights`` maps them: energy rows take ``eweight``, force rows ``fweight``, stress rows ``vweight``, any
        other row type 0."""
        S = np.zeros((len(cands), self.ncat))
        for p, table in enumerate(cands):
            for c, (group, _, row_type) in enumerate(self.keys):
                field = ROW_TYPE_WEIGHT.get(row_type)
                S[p, c] = float(table[group][field]) if field is not None else 0.0
        return S

    def row_weights(self, s):
        """Full row weights w0 * s[category] of one candidate (0 for rows without a category)."""
        s = np.asarray(s, dtype=np.float64)
        return np.where(self.cat >= 0, self.w0 * s[np.maximum(self.cat, 0)], 0.0)

    def _kind(self):
        from .ridge import RIDGE

        if isinstance(self.solver, RIDGE):
            sec = self.solver.config.sections["RIDGE"]
            kind = _capi.SOLVE_RIDGE_INV if bool(sec.local_solver) else _capi.SOLVE_RIDGE
            return kind, float(sec.alpha), False
        return _capi.SOLVE_LSTSQ, self.solver.RCOND, bool(self.solver.row_space)

    def _push_base(self):
        """The rows and the base weights resident on this rank's GPU (no copy when they already are)."""
        if self.m == 0:
            return self.pt.hip()
        ctx = self.solver._upload(self.a, self.b, self._shared)
        mask = (~self.testing).astype(np.uint8)
        ctx.set_weights(self.w0, None if mask.all() else mask)
        return ctx

    def _device(self):
        """The category layout and the per-category statistics (one pass over the rows) on this rank's GPU: prepared on
        first use and again whenever the context no longer holds THIS object's layout -- a context holds one, so another
        CandidateFits on the same solver replaces it, and any new upload of rows drops it.  Collective in a multi-rank
        job: the ranks agree on whether to prepare."""
        ctx = self.pt.hip()
        stale = self._layout is None or ctx.cat_info()["layout"] != self._layout
        if self.pt.multi:
            flag = np.array([1.0 if stale else 0.0])
            self.pt.allreduce_host(flag, _capi.REDUCE_MAX)
            stale = bool(flag[0] > 0)
        if stale:
            layout = 0
            if self.m > 0:
                ctx = self._push_base()
                layout = ctx.cat_prepare(self.cat, self.ncat)
            if self.pt.multi:
                layout, self._stats = ctx.cat_normal_eq_dist(layout, self.K, self.ncat)
            else:
                self._stats = ctx.cat_normal_eq(layout)
            self._layout = layout
        return ctx

    def _cv_device(self, ccat, F):
        """The composite layout fold x category of ``cross_validate`` and its statistics on this rank's GPU, under its own
        tag (``self._cv``, next to ``self._layout``): prepared again whenever the context holds another layout or the folds
        changed.  Collective in a multi-rank job, as ``_device`` is."""
        ctx = self.pt.hip()
        held = self._cv
        stale = (held is None or held[2] != F or ctx.cat_info()["layout"] != held[0]
                 or not (held[1] is ccat or np.array_equal(held[1], ccat)))
        if self.pt.multi:
            flag = np.array([1.0 if stale else 0.0])
            self.pt.allreduce_host(flag, _capi.REDUCE_MAX)
            stale = bool(flag[0] > 0)
        if stale:
            tag = 0
            if self.m > 0:
                ctx = self._push_base()
                tag = ctx.cat_prepare(ccat, F * self.ncat)
            if self.pt.multi:
                tag, ptr = ctx.cat_normal_eq_dist(tag, self.K, F * self.ncat)
            else:
                ptr = ctx.cat_normal_eq(tag)
            self._cv = (tag, ccat, F, ptr)
        return ctx

    def cross_validate(self, S, folds=5, by="Configs", seed=0, method="auto"):
        """Grouped K-fold cross-validation of the candidates S (P x ncat): the units ``fs_dict[by]`` of the training rows
        are dealt into folds (``folds``: an int F, ``None`` for one fold per unit, or a mapping unit -> fold; ``seed`` as in
        ``folds.deal_folds``), every candidate is refitted with each fold left out, and every training row is scored
        under the refit that did not see its unit.  Returns a ``CandidateCV`` (solvers/candidates_cv.py): ``coef`` (P, F, K),
        ``status``, ``min_pivot``, ``route``, ``fold_of_unit``, pooled ``sums`` (P, ncat, 5), ``tables()``,
        ``row_type_errors`` and ``cost(weights, metric)`` -- the weight search's objective on held-out rows.

        The refits are plain Jacobi-scaled Cholesky solves of the normal equations (alpha = [RIDGE] alpha, 0 for SVD); they
        are not ``fit``'s chain of probe, refinement and row-space fallback.  ``method="device"``: kernels V1 + V2 of
        csrc/fsnap_cv.hip (K <= 144), failed problems stay NaN with status 1; ``"composed"``: ``fsnap_fit_candidates`` on
        the composite layout with scales that are zero on the held-out fold, then ``fsnap_candidate_rows``; ``"auto"``: the
        device route with its status-1 problems solved again by the composed one, the composed route beyond 144 columns.

        A context holds ONE category layout: this call prepares the composite layout fold x category under its own tag, and
        the next ``fit`` / ``errors`` prepares this object's own layout again.  Repeated calls with the same folds reuse the
        composite layout and its statistics.  Collective in a multi-rank job: a unit gets one fold on every rank, the
        statistics are summed over the ranks and so are the pooled sums, on every rank.  KeyError without ``fs_dict[by]``;
        ValueError when F x ncat blocks of statistics pass FSNAP_CAT_STATS_MAX_BYTES."""
        from . import candidates_cv

        return candidates_cv.cross_validate(self, S, folds, by, seed, method)

    def cross_validate_gradient(self, S, weights, metric="rmse", folds=5, by="Configs", seed=0, method="auto"):
        """The cross-validated cost of the candidates S (P x ncat) and its exact gradient over S (solvers/candidates_cv_grad.py).
        The cost is J[p] = sum_t weights[t] phi(E[p, t] / n_t) over the row types, E the BASE-weighted held-out sum (w0 r)^2 of
        the training rows of type t (no scaling by S), phi = sqrt for ``metric="rmse"``, the identity for ``"mse"``; with
        w0 = 1 it is ``cross_validate(S).cost(weights, "rmse")`` exactly.  The S-scaled sums are not used: they go to 0 with S.
        ``weights``, ``folds``, ``by``, ``seed`` as in ``cross_validate`` / ``CandidateCV.cost``.

        Returns a ``CandidateCVGradient``: ``cv`` (the ``CandidateCV`` of the same call, device route up to 144 columns),
        ``cost`` (P,), ``grad_S`` = dJ/dS and ``grad_log`` = dJ/dlog|S| (P, ncat), ``grad_log_alpha`` (P,) = dJ/dlog alpha
        ([RIDGE] alpha; 0 for SVD), ``omega``, ``status`` (P, F).  The gradient is the adjoint of the K x K Cholesky solve of
        every refit on its live columns, the live set treated as fixed: one more solve per fold and two sweeps over the
        per-(fold, category) blocks for all ncat derivatives.  ``method="device"``: ``fsnap_cv_candidates_grad`` (kernels G1, G2
        of csrc/fsnap_cvgrad.hip, K <= 144); ``"host"``: the numpy restatement from the downloaded blocks; ``"auto"``: the
        device up to 144 columns, the host beyond.  A candidate with any status-1 fold has NaN cost and a NaN gradient row
        under every method: the adjoint of the truncating composed solve that ``cross_validate(method="auto")`` falls back to
        is not defined here.  Collective in a multi-rank job; every rank returns the same bits.  Like ``cross_validate`` the
        call leaves the composite layout on the context."""
        from . import candidates_cv_grad

        return candidates_cv_grad.cross_validate_gradient(self, S, weights, metric, folds, by, seed, method)

    def descend_weights(self, S0, weights, metric="rmse", steps=20, folds=5, by="Configs", seed=0, eta0=0.5, c1=1e-4,
                        max_halvings=8):
        """Batched steepest descent of the cross-validated cost on theta = log|S| from the P starts S0 (P x ncat) at once: per
        iteration one ``cross_validate_gradient`` call, then line-search rounds of one ``cross_validate`` call over the P trial
        points S exp(-eta grad_log).  Candidate p accepts a trial when its cost is <= cost_p - c1 eta_p |grad_log_p|^2 (Armijo);
        otherwise eta_p is halved, at most ``max_halvings`` times per iteration; eta_p doubles after an accepted step.
        Categories with S = 0 stay 0 (their log-gradient is 0), signs are kept, a candidate with a NaN cost stays where it is.
        Returns (S (P, ncat), cost history (steps + 1, P), accepted step sizes (steps, P), 0 where no step was taken).
        Deterministic and collective.  Deliberately plain: no L-BFGS, no bounds, no step over alpha."""
        from . import candidates_cv_grad

        return candidates_cv_grad.descend_weights(self, S0, weights, metric, steps, folds, by, seed, eta0, c1, max_halvings)

    def evidence(self, S, alpha=None, scale="profiled", method="auto"):
        """The marginal likelihood (type-II likelihood, evidence) of the candidates S (P x ncat) and its exact gradient over all
        category scales (solvers/candidates_evidence.py), the weights w0 S[p, category] read as inverse noise standard
        deviations.  ``alpha=None`` takes [RIDGE] alpha for RIDGE and 0 for SVD; with alpha > 0 it is MacKay's evidence under
        the prior beta ~ N(0, 1 / alpha), with alpha = 0 the restricted likelihood of a variance-components model with one
        component per category.  ``scale="fixed"``: unit noise scale; ``"profiled"``: a common noise scale sigma^2 maximised
        out.  Returns a ``CandidateEvidence``: ``log_evidence``, ``beta``, ``logdet``, ``sigma2``, ``rss``, ``dof``, ``noise``
        (= rss / (n - dof) per category), ``grad_logS``, ``grad_logalpha``, ``live``, ``status``, ``min_pivot``.  No folds and
        no pass over the rows: everything comes from the per-category statistics ``fit`` uses.

        The solve is a plain Jacobi-scaled Cholesky of the normal equations on the live columns (``cross_validate``'s, not
        ``fit``'s chain); a candidate with a scaled pivot not above 1e-10 has status 1 and NaN in every field, no other
        candidate changes.  ``method="device"``: ``fsnap_candidates_evidence`` (kernels E1-E3 of csrc/fsnap_evidence.hip,
        K <= 144, else ValueError); ``"host"``: numpy on the downloaded blocks; ``"auto"``: the device up to 144 columns, the
        host beyond.  Collective in a multi-rank job (the statistics are already summed over the ranks): every rank returns
        the same bits.  The layout and its statistics are not touched."""
        from . import candidates_evidence

        return candidates_evidence.evidence(self, S, alpha, scale, method)

    def maximise_evidence(self, S0, alpha=None, scale="profiled", steps=50, tol=1e-6, damping=1.0, method="auto"):
        """Batched fixed-point ascent of the evidence on theta = log|S| from the P starts S0 (P x ncat) at once: per iteration
        one ``evidence`` call, then trial calls for the safeguard.  The step is theta_c += eta / 2 log((n_c - gamma_c) /
        (kappa lambda_c Q_c)) on the active categories whose numerator and denominator are positive; candidate p accepts it
        only if its L does not decrease, otherwise eta_p is halved, at most 8 times; after an accepted step eta_p doubles up to
        ``damping``.  S = 0 stays 0, signs are kept, a NaN candidate is left alone.  A candidate stops when
        max_c |dL/dlog S[p, c]| / n_c <= ``tol``.  Returns (S (P, ncat), the ``CandidateEvidence`` there, the accepted L per
        iteration (iterations + 1, P), converged (P,) bool).  alpha is NOT stepped: it stays what the call was given."""
        from . import candidates_evidence

        return candidates_evidence.maximise_evidence(self, S0, alpha, scale, steps, tol, damping, method)

    # ------------------------------------------------------------------------------
    def fit(self, S):
        """(P, K) coefficients of the candidates S (P x ncat); ``info`` gets one dict per candidate: rank, rcond,
        refine_steps, path ("statistics" | "row_space")."""
        S = check_scales(S, self.ncat)
        P, K = S.shape[0], self.K
        kind, param, row_space = self._kind()
        probe = _capi.PROBE_OF[kind]
        ctx = self._device()
        betas, ranks, rconds, dptr = ctx.fit_candidates(self._layout, probe, param, S, K)
        T = K * K + K + 3
        self._packed = (ctx, dptr, K, P)
        self.info = [None] * P
        ranks = [int(r) for r in ranks]
        rconds = [float(r) for r in rconds]
        solver = self.solver
        on_gpu = (self.pt.comm_kind != "torch" or not self.pt.multi)
        row_space_fits = []
        refine = []
        for p in range(P):
            ptr = dptr + p * T * 8
            rank, rcond = ranks[p], rconds[p]
            if row_space and on_gpu and self._needs_row_space(ctx, ptr, rank, rcond):
                row_space_fits.append(p)
                continue
            if rank < 0:          # Solver._resolve_probe: the truncating solve on the downloaded statistics
                G, c, _ = ctx.download_packed(ptr, K)
                betas[p] = solver._solve(kind, param, G, c)
                rank = int(solver.last_rank)
            self.info[p] = {"rank": rank, "rcond": rcond, "refine_steps": 0, "path": "statistics"}
            if solver.refine_steps and rank == K and not refinement_skip(K, rcond):
                refine.append(p)
        if refine:
            self._refine(ctx, betas, S, refine, dptr, T, kind, param, rconds)
        for p in row_space_fits:
            betas[p] = self._row_space_fit(S[p])
            self.info[p] = {"rank": int(solver.last_rank), "rcond": rconds[p], "refine_steps": 0, "path": "row_space"}
        if row_space_fits:
            self._push_base()     # the resident base weights again, for later candidates and errors()
        return betas

    def candidate_statistics(self, p):
        """(G, c, scalars) of candidate p of the last ``fit`` -- the combined statistics its solve started from, as
        ``solver.last_statistics`` holds them after a single fit.  Valid until the next ``fit``."""
        if getattr(self, "_packed", None) is None:
            raise RuntimeError("no fit yet")
        ctx, dptr, K, P = self._packed
        if not 0 <= p < P:
            raise IndexError(f"candidate {p} of {P}")
        return ctx.download_packed(dptr + p * (K * K + K + 3) * 8, K)

    def _needs_row_space(self, ctx, ptr, rank, rcond):
        """Solver._needs_row_space for one candidate's solve (same rule, same constants)."""
        if rcond is None:
            return False
        if rank < 0:
            return True
        ill = rcond / RCOND_MARGIN < self.solver.ROWSPACE_RCOND
        if rank < self.K:
            G = ctx.download_packed(ptr, self.K)[0]
            zero_cols = int(np.count_nonzero(np.diag(G) == 0.0))
            return rank < self.K - zero_cols or ill
        return ill

    def _refine(self, ctx, betas, S, todo, dptr, T, kind, param, rconds):
        """Solver._refine for every candidate in ``todo`` at once: one pass over the rows per step for all candidates
        still refining (``fsnap_candidate_rows``), then one K x K solve each."""
        K = self.K
        alpha = param if kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_RIDGE_INV) else 0.0
        prev = {p: float(np.max(np.abs(betas[p]))) if K else 0.0 for p in todo}
        active = list(todo)
        for _ in range(int(self.solver.refine_steps)):
            if not active:
                break
            if self.m > 0:
                s = ctx.candidate_rows(self._layout, betas[active], S[active], _capi.CAND_RHS, self.ncat)
            else:
                s = np.zeros((len(active), K))
            if self.pt.multi:
                s = np.ascontiguousarray(s)
                self.pt.allreduce_host(s.reshape(-1))
            still = []
            for i, p in enumerate(active):
                rhs = s[i] - alpha * betas[p]
                delta, rank, _ = ctx.solve_device(kind, param, K, dptr + p * T * 8, rhs=rhs)
                if rank < K:
                    continue
                betas[p] = betas[p] + delta
                self.info[p]["refine_steps"] += 1
                step = float(np.max(np.abs(delta)))
                if refinement_done(K, step, prev[p], float(np.max(np.abs(betas[p]))), rconds[p]):
                    continue
                prev[p] = step
                still.append(p)
            active = still

    def _row_space_fit(self, s):
        """The solver's own single-candidate path with the full row weights of the candidate (collective)."""
        solver = self.solver
        saved = solver.fit
        w = self.row_weights(s)
        fs = dict(self.fs_dict)
        # the rows are this object's own, resident since _device: keep_resident lets perform_fit see that instead of
        # uploading them again (which would also drop the category layout)
        keep = solver.keep_resident
        solver.keep_resident = True
        try:
            solver.perform_fit(self.a, self.b, w[~self.testing], fs_dict=fs)
        finally:
            solver.keep_resident = keep
        beta = solver.fit
        if self.pt.multi:
            beta = self.pt.bcast_object(beta, src=0)
        solver.fit = saved
        return np.asarray(beta, dtype=np.float64).reshape(-1)

    # ------------------------------------------------------------------------------
    def error_sums(self, betas, S):
        """(P, ncat, 10) sums of ``fsnap_error_stats`` of this rank's rows for every candidate."""
        S = check_scales(S, self.ncat)
        betas = np.ascontiguousarray(betas, dtype=np.float64).reshape(S.shape[0], -1)
        if betas.shape[1] != self.K:
            raise ValueError(f"betas must have shape (P, {self.K})")
        ctx = self._device()                                  # collective: every rank, rows or not
        if self.m > 0:
            sums4 = ctx.candidate_rows(self._layout, betas, None, _capi.CAND_ERROR_SUMS, self.ncat)
        else:
            sums4 = np.zeros((S.shape[0], self.ncat, 4))
        return np.array([assemble_sums(self.const, sums4[p], S[p]) for p in range(S.shape[0])])

    def errors(self, betas, S, frames=True):
        """Error tables of the candidates: a list of P DataFrames laid out exactly like ``solver.errors``, or with
        ``frames=False`` P pairs (per-group metrics (ncat, 8), *ALL metrics (n, 8)) of arrays, columns ncount, mae, rmse,
        rsq, w_ncount, w_mae, w_rmse, w_rsq, rows in ``keys`` order.  Multi-rank: collective, ``None`` on ranks > 0."""
        st = self.error_sums(betas, S)
        solver = self.solver
        if self.pt.multi:
            tables = solver._allgather_tables(st)                  # (ranks, P, ncat, 10)
            if self.pt._rank != 0:
                return None
            st = np.array([[solver._pool_sums(rows[rows[:, 0] > 0]) for rows in np.swapaxes(tables[:, p], 0, 1)]
                           for p in range(st.shape[0])]).reshape(st.shape)
        out = []
        for p in range(st.shape[0]):
            if not frames:
                out.append(solver._metric_arrays(self.keys, st[p]))
                continue
            lay = solver._err_layout
            if lay is not None and lay[0] is self.keys:
                grouped, allrows = solver._metric_arrays(self.keys, st[p])
                if lay[4] != (len(allrows), len(grouped)):
                    grouped, allrows = solver._tables_from_sums(self.keys, st[p])
            else:
                grouped, allrows = solver._tables_from_sums(self.keys, st[p])
            out.append(solver._assemble_errors(grouped, allrows, self.keys))
        return out
