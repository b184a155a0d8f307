"""ARD solver behind the reference's plugin API (fitsnap3lib/solvers/ard.py:9-49).

The reference hands the weighted m x K matrix to scikit-learn's ``ARDRegression``; every
iteration of that algorithm touches the data only through ``X_keep.T X_keep``,
``X_keep.T y`` and the residual sum of squares (sklearn 1.7.2 linear_model/_bayes.py,
``ARDRegression.fit`` / ``_update_sigma``).  Here the first two come once from the GPU
statistics (G, c) and the third from the streaming GEMV+SSE kernel each iteration, so the
loop below is a sufficient-statistics restatement of that algorithm with K x K host
algebra.  The reference's class spells the iteration cap ``n_iter=`` (ard.py:40-45), which
scikit-learn >= 1.5 no longer accepts; the goldens come from that class run with the keyword
forwarded as ``max_iter`` (tests/golden/make_golden.py).  Accuracy: the K x K inverse of every
iteration is taken of the column-EQUILIBRATED matrix, which puts the result within 1e-6
(element-wise) of the iteration carried out in extended precision; the reference class's own
float64 vectors are 3e-4 from that yardstick (its ``pinvh`` works on columns that span 15
decades), and that -- not this solver -- is what separates the two: equal support, and a
distance to the goldens no larger than the goldens' own distance to the extended-precision
result (tests/test_host_logic.py, tests/test_gpu_parity.py: all rows / a testing mask /
directmethod / non-default scap, scai, logcut)."""
from __future__ import annotations

import numpy as np
from scipy.linalg import pinvh

from .._hostblas import blas_threads
from .solver import Solver


class ARD(Solver):

    TOL = 1.0e-3        # ARDRegression default `tol`
    MAX_ITER = 1000     # ard.py:40-45 (n_iter=1000)

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.exact_sse = True   # recompute sum((y - X beta)^2) on the GPU each iteration (sklearn does)
        self.n_iter_ = None
        self.lambda_ = None
        self.alpha_ = None

    def perform_fit(self):
        """ard.py:15-49 — no arguments: data comes from ``pt.shared_arrays``."""
        pt = self.pt
        G, c, s = self._fit_statistics(None, None, None, None, False)
        bb, sbw, n = float(s[0]), float(s[1]), float(s[2])
        var_bw = bb / n - (sbw / n) ** 2
        host_sse = None
        if self.config.sections["EXTRAS"].apply_transpose:
            # ard.py:22-24: X = aw.T aw = G, y = aw.T bw = c -- the loop then runs on (G.T G, G.T c) with K "samples",
            # and the residual of an iteration is the K-vector c - G coef (host)
            X, y = G, c
            G, c = X.T @ X, X.T @ y
            bb, n, var_bw = float(y @ y), float(len(y)), float(np.var(y))
            host_sse = lambda coef: float(np.sum((y - X @ coef) ** 2))    # noqa: E731
        ap = 1.0 / var_bw
        sec = self.config.sections["ARD"]
        pt.single_print("inverse variance in training data: %f, logscale for threshold_lambda: %f" % (ap, np.log10(ap)))
        pt.single_print("automated threshold_lambda will be 10**(%f + %1.3f)" % (sec.logcut, np.abs(np.log10(ap))))
        if sec.directmethod:
            hyper = dict(threshold_lambda=sec.threshold_lambda, alpha_1=sec.alphabig, alpha_2=sec.alphabig,
                         lambda_1=sec.lambdasmall, lambda_2=sec.lambdasmall)
        else:
            hyper = dict(alpha_1=sec.scap * ap, alpha_2=sec.scap * ap, lambda_1=ap * sec.scai, lambda_2=ap * sec.scai,
                         threshold_lambda=10 ** (int(np.abs(np.log10(ap))) + sec.logcut))
        coef = self._ard_loop(G, c, bb, n, var_bw, host_sse=host_sse, **hyper)
        if pt._rank == 0:
            self.fit = coef

    # sklearn 1.7.2 linear_model/_bayes.py ARDRegression.fit, on (G, c) instead of (X, y)
    # ``live`` (columns that may ever be kept), ``tol`` / ``max_iter`` (default: the class constants), ``alpha_init`` (default
    # 1 / (var_y + eps)) and ``probe`` serve solvers/ard_path.py; their defaults leave the loop, and its bits, as perform_fit
    # runs it.  With a ``probe`` dict the loop reports into it -- "status" (0 converged or emptied, 1 failed, 2 max_iter
    # reached), "delta" (the last sum |coef_old - coef|, against zeros in iteration 0), "pivot" (the smallest Cholesky pivot of
    # the scaled matrices) -- and a scaled matrix that is not positive definite or a non-finite lambda ends it with status 1
    # and NaN coefficients instead of being divided through.
    def _ard_loop(self, G, c, bb, n_samples, var_y, alpha_1, alpha_2, lambda_1, lambda_2, threshold_lambda, host_sse=None,
                  live=None, tol=None, max_iter=None, alpha_init=None, probe=None):
        K = len(c)
        eps = np.finfo(np.float64).eps
        coef_ = np.zeros(K)
        keep = np.ones(K, dtype=bool) if live is None else np.array(live, dtype=bool)
        alpha_ = 1.0 / (var_y + eps) if alpha_init is None else float(alpha_init)
        tol = self.TOL if tol is None else tol
        max_iter = self.MAX_ITER if max_iter is None else max_iter
        lambda_ = np.ones(K)
        coef_old = None

        # sigma = (diag(lambda) + alpha G)^-1 through the column-equilibrated matrix:
        #   sigma = D^-1 (D^-1 diag(lambda) D^-1 + alpha D^-1 G D^-1)^-1 D^-1,   D = diag(sqrt(G_jj)).
        # scikit-learn inverts the unscaled matrix (``pinvh(lambda I + alpha X^T X)``); with descriptor columns that span
        # 15 decades that loses kappa(G) eps -- its own float64 answer on the Ta rows sits 3e-4 (element-wise) from the
        # same iteration carried out in extended precision, this form 5e-7 (oracle.ard_fit_extended, tests)
        dsc = np.sqrt(np.diag(G))
        dsc[~(dsc > 0.0)] = 1.0
        Gh = G / np.outer(dsc, dsc)

        def update_sigma(alpha_, lambda_, keep):
            dk = dsc[keep]
            with blas_threads(len(dk)):         # (an eigh of <= K x K: the BLAS pool sized by the CPUs it sees takes 20 x longer)
                scaled = np.diag(lambda_[keep] / dk ** 2) + alpha_ * Gh[np.ix_(keep, keep)]
                if probe is not None:
                    piv = np.linalg.cholesky(scaled).diagonal() ** 2        # LinAlgError: not positive definite
                    probe["pivot"] = min(probe.get("pivot", np.inf), float(piv.min()))
                scaled = pinvh(scaled)
            return scaled / np.outer(dk, dk)

        def sse_of(coef_):
            if host_sse is not None:
                return host_sse(coef_)
            if self.exact_sse:
                return self._device_sse(coef_)
            return float(bb - 2.0 * coef_ @ c + coef_ @ G @ coef_)

        n_iter, status = 0, 2
        if probe is not None:
            probe.update(status=0, delta=np.inf, pivot=np.inf)
            coef_old = np.zeros(K)
        try:
            for it in range(max_iter if (live is None or keep.any()) else 0):
                n_iter = it + 1
                sigma_ = update_sigma(alpha_, lambda_, keep)
                coef_[keep] = alpha_ * (sigma_ @ c[keep])
                sse_ = sse_of(coef_)
                gamma_ = 1.0 - lambda_[keep] * np.diag(sigma_)
                lambda_[keep] = (gamma_ + 2.0 * lambda_1) / (coef_[keep] ** 2 + 2.0 * lambda_2)
                alpha_ = (n_samples - gamma_.sum() + 2.0 * alpha_1) / (sse_ + 2.0 * alpha_2)
                if probe is not None and not (np.all(np.isfinite(lambda_)) and np.isfinite(alpha_)):
                    raise np.linalg.LinAlgError("non-finite lambda or alpha")
                keep = lambda_ < threshold_lambda
                if live is not None:
                    keep &= live
                coef_[~keep] = 0
                if probe is not None:
                    probe["delta"] = float(np.sum(np.abs(coef_old - coef_)))
                if it > 0 and np.sum(np.abs(coef_old - coef_)) < tol:
                    status = 0
                    break
                coef_old = np.copy(coef_)
                if not keep.any():
                    status = 0
                    break
            if n_iter == 0:
                status = 0                      # no live column: nothing to iterate
            self.n_iter_ = n_iter
            if keep.any():
                sigma_ = update_sigma(alpha_, lambda_, keep)
                coef_[keep] = alpha_ * (sigma_ @ c[keep])
        except np.linalg.LinAlgError:
            if probe is None:
                raise
            self.n_iter_ = n_iter
            status = 1
            coef_ = np.full(K, np.nan)
        if probe is not None:
            probe["status"] = status
        self.lambda_, self.alpha_ = lambda_, alpha_
        return coef_

    def _device_sse(self, coef_):
        """sum over training rows of (w (b - A coef))^2 on every rank's rows, summed over ranks."""
        pt = self.pt
        ctx = pt.hip()
        _, sse = ctx.predict(coef_, want_preds=False, want_sse=True)
        return pt.allreduce_scalar(sse)
