"""ANL (analytical Bayesian linear fit) behind the reference's plugin API
(fitsnap3lib/solvers/anl.py:7-68): posterior mean ``pinv(aw.T aw + nugget I) aw.T bw`` and
covariance ``sigma_hat * pinv(...)`` — another consumer of the same GPU statistics (G, c)
plus one streamed residual pass (``fsnap_predict``'s weighted SSE).  The K x K pseudo-inverse
is host algebra, as in the reference."""
from __future__ import annotations

import numpy as np

from .._hostblas import blas_threads
from .solver import Solver


class ANL(Solver):

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.save_files = True      # the reference writes covariance.npy / mean.npy into the cwd (anl.py:60-61)

    def perform_fit(self, a=None, b=None, w=None, trainall=False):
        pt, config = self.pt, self.config
        G, c, s = self._fit_statistics(a, b, w, None, trainall)
        nbas = len(c)
        npt = float(s[2])
        cov_nugget = config.sections["SOLVER"].cov_nugget
        transposed = config.sections["EXTRAS"].apply_transpose and transpose_trick_ok(G)
        invptp, fit, sse = posterior_noise(pt, G, c, cov_nugget, transposed)
        if transposed:
            npt = float(nbas)                       # the "rows" of the transposed system
        bp = sse / 2.0
        ap = (npt - nbas) / 2.0
        sigmahat = bp / (ap - 1.0)
        self.sigmahat = float(sigmahat)             # the noise variance Solver.select_batch conditions on
        if pt._rank != 0:
            return
        self.fit = fit
        self.cov = sigmahat * invptp                                                # anl.py:53
        if self.save_files:
            np.save("covariance.npy", self.cov)
            np.save("mean.npy", self.fit)
        nsam = config.sections["SOLVER"].nsam
        if nsam:
            self.fit_sam = np.random.multivariate_normal(self.fit, self.cov, size=(nsam,))   # anl.py:63-65


def transpose_trick_ok(G):
    """anl.py:31-36 / merr.py:19-24: the regression may run on (aw.T aw, aw.T bw) = (G, c) instead of the rows when
    cond(aw)^2 = lambda_max(G) / lambda_min(G) < 1 / eps -- K x K host algebra on the statistics."""
    with blas_threads(G.shape[0]):
        ev = np.linalg.eigvalsh(G)
    if abs(ev[-1]) / max(abs(ev[0]), np.finfo(float).tiny) < 1.0 / np.finfo(float).eps:
        return True
    print("The Matrix is ill-conditioned for the transpose trick")
    return False


def posterior_noise(pt, G, c, cov_nugget, transposed, keep=None):
    """The analytical posterior of ANL (anl.py:38-50, merr.py:39-50): ``invptp = pinv(P + nugget I)`` symmetrised, the
    mean ``fit`` and the weighted residual sum of squares ``sse`` of the regression on the columns ``keep`` (a boolean
    mask; None = all).  P = G[keep, keep] on the rows, whose exact residual is one streamed pass over them on the GPU
    (``fsnap_predict``, summed over the ranks); with ``transposed`` the "rows" are (G[:, keep], c), all host algebra.
    Returns (invptp, fit over the kept columns, sse)."""
    if transposed:
        Gc = G if keep is None else G[:, keep]
        nbas = Gc.shape[1]
        with blas_threads(nbas):
            invptp = np.linalg.pinv(Gc.T @ Gc + cov_nugget * np.diag(np.ones((nbas,))))
        invptp = invptp * 0.5 + invptp.T * 0.5
        fit = np.dot(invptp, Gc.T @ c)
        res = c - Gc @ fit
        return invptp, fit, float(res @ res)
    Gk = G if keep is None else G[np.ix_(keep, keep)]
    ck = c if keep is None else c[keep]
    nbas = len(ck)
    with blas_threads(nbas):            # (an SVD of K x K: _hostblas.py)
        invptp = np.linalg.pinv(Gk + cov_nugget * np.diag(np.ones((nbas,))))       # anl.py:39
    invptp = invptp * 0.5 + invptp.T * 0.5                                        # anl.py:40
    fit = np.dot(invptp, ck)
    full = fit
    if keep is not None:
        full = np.zeros(len(c))
        full[keep] = fit
    # res = bw - aw @ fit; bp = res.res / 2  (anl.py:46-47): exact streamed residual on the GPU
    _, sse = pt.hip().predict(full, want_preds=False, want_sse=True)
    return invptp, fit, pt.allreduce_scalar(sse)
