"""MERR (model-error embedding) behind the reference's plugin API (fitsnap3lib/solvers/merr.py:14-88 with
lreg.py:66-195 ``lreg_merr``): a maximum-a-posteriori fit of the coefficients together with the spread ``sigma`` of
an embedded model error, by BFGS on the log-posterior ``logpost_emb``.  Unlike the other linear solvers it does not
reduce to the statistics (G, c): its per-row variance ``v_i = sum_{j in E} (x_ij sigma_j)^2 + d`` makes every
evaluation read all rows.  Each evaluation is one fused pass over the resident rows on the GPU (``fsnap_merr_eval``)
that returns the log-posterior AND its exact gradient -- the reference hands BFGS no gradient and pays K + |E| + 1
numpy passes per finite-difference gradient.  The trajectories therefore differ; the log-posterior reached is the
comparable quantity (an equal or higher one).

Several ranks: BFGS runs on every rank and must stay in lockstep, since each evaluation is a collective.  So every
input of the optimiser is rank 0's: the start (its random draw included) and the data variance are broadcast from
rank 0, each rank evaluates its own rows, and the [val | g | h] sums are all-reduced and then broadcast from rank 0.
With the same start and the same bits of every value and gradient, the ranks take the same steps (the reference runs
MERR on rank 0 only)."""
from __future__ import annotations

import numpy as np
from scipy.optimize import minimize

from .. import _capi
from .._hostblas import blas_threads
from .anl import posterior_noise, transpose_trick_ok
from .solver import Solver

ABC_EPS = 0.1           # lreg.py: abceps


def merr_constant(method, npt):
    """The log-posterior's constant terms (lreg.py logpost_emb): -n log(2 pi) / 2 for iid / full, once
    -log(2 pi) / 2 - log(eps) for abc."""
    if method == "abc":
        return -0.5 * np.log(2.0 * np.pi) - np.log(ABC_EPS)
    return -0.5 * npt * np.log(2.0 * np.pi)


def merr_q(cf, sig, emb, multiplicative):
    """q_j = sum of sigma_k^2 over the embedded slots k of column j (sigma_k = |c_j| s_k when multiplicative)."""
    sigma = np.abs(cf[emb]) * sig if multiplicative else sig
    q = np.zeros(len(cf))
    np.add.at(q, emb, sigma * sigma)
    return q


def merr_gradient(cf, sig, emb, multiplicative, g, h):
    """(dL/dc over all columns, dL/ds) from the pass's sums g = sum dl/de x_i, h = sum dl/dv x_i o x_i:
    additive dL/dc = g, dL/ds_k = 2 s_k h_j; multiplicative (sigma_k = |c_j| s_k)
    dL/dc_j = g_j + sum_k 2 c_j s_k^2 h_j, dL/ds_k = 2 s_k c_j^2 h_j (j = emb[k])."""
    hj = h[emb]
    if multiplicative:
        cj = cf[emb]
        gc = np.array(g, dtype=np.float64)
        np.add.at(gc, emb, 2.0 * cj * sig * sig * hj)
        return gc, 2.0 * sig * cj * cj * hj
    return np.array(g, dtype=np.float64), 2.0 * sig * hj


def embedded_columns(merr_cfs, nbas):
    """merr.py:56-66: 'all' or a space-separated list of indices into the REDUCED columns (zero columns dropped)."""
    if merr_cfs == "all":
        return np.arange(nbas)
    ind = []
    for i in list(merr_cfs.split(" ")):     # sanity check, as the reference (an index == nbas then fails to index)
        assert int(i) <= nbas
        ind.append(int(i))
    return np.array(ind, dtype=np.int64)


class MERR(Solver):

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.save_files = True      # the reference writes covariance.npy / mean.npy into the cwd (merr.py:84-85)

    def perform_fit(self, a=None, b=None, w=None, trainall=False):
        pt, config = self.pt, self.config
        sec = config.sections["SOLVER"]
        method = sec.merr_method
        if method not in _capi.MERR_METHODS:
            raise ValueError(f"Merr type {method} unknown")
        multiplicative = bool(sec.merr_mult)
        G, c, s = self._fit_statistics(a, b, w, None, trainall)
        K = len(c)
        transposed = config.sections["EXTRAS"].apply_transpose and transpose_trick_ok(G)
        # merr.py:28-34: all-zero columns of aw (G_jj = 0) leave the parameter vector; on the device c_j = q_j = 0
        keep = np.diag(G) != 0.0
        cols = np.flatnonzero(keep)
        nbas = len(cols)
        npt = float(K) if transposed else float(s[2])
        invptp, _, sse = posterior_noise(pt, G, c, sec.cov_nugget, transposed, keep)      # merr.py:38-50
        sigmahat = (sse / 2.0) / ((npt - nbas) / 2.0 - 1.0)
        emb = embedded_columns(sec.merr_cfs, nbas)
        emb_full = cols[emb]

        if pt.multi:
            sigmahat = float(pt.bcast_object(float(sigmahat), 0))
        evaluator = _TransposedRows(pt, G, c) if transposed else None
        ctx = evaluator.ctx if transposed else pt.hip()
        reduce_ranks = pt.multi and not transposed
        const = merr_constant(method, npt)

        def neg_logpost(x):
            cf = np.zeros(K)
            cf[cols] = x[:nbas]
            sig = x[nbas:]
            q = merr_q(cf, sig, emb_full, multiplicative)
            if ctx.m > 0:
                val, g, h = ctx.merr_eval(method, cf, q, sigmahat)
            else:
                val, g, h = 0.0, np.zeros(K), np.zeros(K)
            if pt.multi:
                sums = np.concatenate([[val], g, h])
                if reduce_ranks:                         # (transposed: every rank holds the same (G, c) rows)
                    sums = pt.allreduce_host(sums, 0)
                sums = pt.bcast_object(sums, 0)          # every rank on rank 0's bits: the BFGS loops stay in lockstep
                val, g, h = float(sums[0]), sums[1:K + 1], sums[K + 1:]
            gc, gs = merr_gradient(cf, sig, emb_full, multiplicative, g, h)
            self.evaluations += 1
            return -(val + const), -np.concatenate([gc[cols], gs])

        # lreg.py:138-142: random start (numpy's global generator, as the reference), coefficients from the ridged
        # normal equations of the kept columns
        params_ini = np.random.rand(nbas + len(emb))
        if transposed:
            Gc = G[:, keep]
            P, r = Gc.T @ Gc, Gc.T @ c
        else:
            P, r = G[np.ix_(keep, keep)], c[keep]
        with blas_threads(nbas):
            params_ini[:nbas] = np.dot(np.linalg.inv(P + 1.e-6 * np.diag(np.ones((nbas,)))), r)
        if pt.multi:
            params_ini = np.array(pt.bcast_object(params_ini, 0), dtype=np.float64)   # one start for all ranks
        self.objective = neg_logpost       # (-L, -dL/dx) at a parameter vector; collective over the ranks
        try:
            self.evaluations = 0
            self.logpost_ini = -float(neg_logpost(params_ini)[0])      # log-posterior at the start
            self.evaluations = 0
            res = minimize(neg_logpost, params_ini, jac=True, method="BFGS", options={"gtol": 1e-3})   # lreg.py:168
        finally:
            if evaluator is not None:
                evaluator.close()
        self.params_ini = params_ini
        self.params = res.x
        self.logpost = -float(res.fun)
        self.datavar = sigmahat

        coeffs, sig = res.x[:nbas], res.x[nbas:]
        sig_all = np.zeros(nbas)
        sig_all[emb] = np.abs(coeffs[emb]) * sig if multiplicative else sig         # lreg.py:178-182
        fit = np.zeros(K)
        fit[cols] = coeffs
        cov = np.zeros((K, K))
        cov[cols, cols] = sig_all ** 2                                               # merr.py:69-82: backfilled
        self.fit, self.cov = fit, cov
        if pt._rank != 0:
            return
        if self.save_files:
            np.save("covariance.npy", self.cov)
            np.save("mean.npy", self.fit)
        nsam = sec.nsam
        if nsam:
            self.fit_sam = np.random.multivariate_normal(self.fit, self.cov, size=(nsam,))


class _TransposedRows:
    """apply_transpose: the "rows" of the regression are (G, c) with unit weights (merr.py:19-24).  They get a context
    of their own on this rank's device, so the resident training rows stay as they are."""

    def __init__(self, pt, G, c):
        self.ctx = _capi.HipContext(pt.device_index())
        self.ctx.upload_rows(np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64))
        self.ctx.set_weights(np.ones(len(c)))

    def close(self):
        self.ctx.close()
