"""OMP solver: the least-squares fit on the best ``terms`` columns, chosen greedily (no counterpart in the reference).

Forward selection -- orthogonal matching pursuit, or its orthogonal-least-squares form -- touches the rows only through
``X^T X``, ``X^T y`` and ``|y|^2``.  Here those three come from ONE pass of the fused GPU statistics kernel (summed over the
ranks) and the selection runs on the K x K statistics inside the library (``fsnap_omp_gram``): a Cholesky factorisation whose
pivot is chosen by ``[OMP] criterion`` after the ``[OMP] forced`` columns, stopped after ``[OMP] terms`` steps.  The fit is
the unshrunk least-squares solution on the chosen columns and an exact zero on every other, so the cost of evaluating the
potential falls with the columns dropped.  ``Solver.omp_path`` cross-validates the number of terms."""
from __future__ import annotations

from .. import _capi
from .solver import Solver


class OMP(Solver):

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.order = None       # the columns in the order they were chosen (-1 once no candidate was left)
        self.path = None        # per step: weighted squared training error, score and pivot of the chosen column

    def perform_fit(self):
        """No arguments: data comes from ``pt.shared_arrays``."""
        pt = self.pt
        G, c, s = self._fit_statistics(None, None, None, None, False)
        y_norm2 = float(s[0])
        if self.config.sections["EXTRAS"].apply_transpose:
            # as LASSO does: X = aw.T aw = G (K "samples"), y = aw.T bw = c
            X, y = G, c
            G, c = X.T @ X, X.T @ y
            y_norm2 = float(y @ y)
        sec = self.config.sections["OMP"]
        K = G.shape[0]
        terms = sec.terms if sec.terms > 0 else K
        if terms > K:
            raise ValueError(f"OMP: terms = {terms} for {K} columns")
        if any(j >= K for j in sec.forced):
            raise ValueError(f"OMP: forced = {list(sec.forced)} for {K} columns")
        self.order, self.path, coef = _capi.omp_gram(G, c, y_norm2, terms, sec.criterion, sec.forced)
        if pt._rank == 0:
            self.fit = coef[-1].copy()
