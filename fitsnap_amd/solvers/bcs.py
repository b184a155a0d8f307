"""BCS solver: Bayesian compressive sensing behind the reference's plugin API (fitsnap3lib/solvers/bcs.py; ``solver = BCS`` in
docs/source/Linear.rst) -- a sparse fit that comes with a posterior covariance on its support.

``bcs()`` is the fast relevance-vector recurrence of Tipping & Faul as coded by Ji: it adds, re-estimates or deletes one column
per iteration, whichever raises the marginal likelihood most.  Like LASSO, ARD and OMP it touches the weighted training rows
only through (A^T A, A^T y, |y|^2, sum y, n), so here those come from ONE pass of the fused GPU statistics kernel (summed over
the ranks) and the recurrence runs on the K x K statistics inside the library (``fsnap_bcs_gram``, include/fsnap_hip.h, which
lists every departure from the reference's text).  ``[BCS]``: ``sigma2`` (the initial noise variance, which sets the sparsity;
blank: ``scale`` x var(bw), the reference's rule with ``scale`` = 0.01), ``eta`` (1e-18, what the reference's solver passes),
``itermax`` (10, the reference's constant), ``max_active`` (0: min(K, 64), what the kernel of ``bcs_path`` holds) and
``deletion``:

  reference  what the reference computes.  Its deletion branch reads ``Sig[:, which]`` through a view which its own in-place
             downdate of ``Sig`` has zeroed, so after a deletion ``mu`` only loses its entry and ``S``, ``Q`` stay stale.  The
             default: a drop-in user gets the same potential file.
  exact      Tipping & Faul's deletion update of ``mu``, ``S`` and ``Q``.

``fit`` is zeros with ``mu`` on the support; ``cov`` = diag(fit^2) with the support block set to ``Sig``, its negative
entries clipped to 0 as the reference clips them; ``fit_sam`` is drawn as the reference draws it (``nsam`` samples from numpy's
global generator; none with ``nsam`` = 0, as ANL).  ``errbars``, ``used``, ``sigma2`` (re-estimated) and ``bcs`` (the whole
``_capi.BcsFit``) are kept as attributes.  ``Solver.bcs_path`` cross-validates ``sigma2`` / ``scale`` and the iteration cap."""
from __future__ import annotations

import numpy as np

from .. import _capi
from .solver import Solver
from .bcs_path import resolve_max_active


def transposed_statistics(G, c):
    """The reference's substitution aw <- aw.T aw, bw <- aw.T bw on the statistics: (G^2, G c, c . c, sum c, K)."""
    return G.T @ G, G.T @ c, float(c @ c), float(np.sum(c)), float(len(c))


def posterior(K, fit):
    """(fit (K), cov (K x K)) of a ``_capi.BcsFit`` as the reference's solver forms them."""
    beta = np.zeros(K)
    beta[fit.active] = fit.mu
    cov = np.diag(beta ** 2)
    cov[np.ix_(fit.active, fit.active)] = np.where(fit.Sig < 0.0, 0.0, fit.Sig)
    return beta, cov


class BCS(Solver):

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.errbars = None     # one standard deviation around the weights of the support, by position
        self.used = None        # the support, in the order the recurrence holds it
        self.sigma2 = None      # the re-estimated noise variance
        self.bcs = None         # the whole _capi.BcsFit of the last fit

    def perform_fit(self, a=None, b=None, w=None, fs_dict=None, trainall=False):
        pt, config = self.pt, self.config
        G, c, s = self._fit_statistics(a, b, w, fs_dict, trainall)
        y2, sum_y, n = float(s[0]), float(s[1]), float(s[2])
        if config.sections["EXTRAS"].apply_transpose:
            G, c, y2, sum_y, n = transposed_statistics(G, c)        # host: K "rows"
        sec = config.sections["BCS"]
        K = G.shape[0]
        fit = _capi.bcs_gram(G, c, y2, sum_y, n, sec.sigma2, sec.scale, sec.eta, sec.itermax, resolve_max_active(sec.max_active, K),
                             sec.deletion)
        if fit.status == 1:
            raise np.linalg.LinAlgError("BCS: the posterior covariance is not positive semi-definite or not finite")
        self.bcs, self.used, self.errbars, self.sigma2 = fit, fit.active, fit.errbars, fit.sigma2
        if pt._rank != 0:
            return
        self.fit, self.cov = posterior(K, fit)
        nsam = config.sections["SOLVER"].nsam
        if nsam:
            self.fit_sam = np.random.multivariate_normal(self.fit, self.cov, size=(nsam,))
