"""Host side of the predictive-variance pass (``fsnap_row_variance``): the small matrix M that turns every method of the
reference's ``Solver._compute_stdev`` (fitsnap3lib/solvers/solver.py:440-472) into one of the kernel's two row forms

    QUAD (M = cov, K x K)   v_i = a_i^T M a_i          fullcov, loop
    NORM (M: K x J)         v_i = ||a_i M||^2          chol (M = L), choleye (shifted L), svd (M = U sqrt(S)),
                                                       sam (M = (X - mean)^T / sqrt(nsam), X the nsam x K samples)

and stdev = sqrt(v).  ``sam`` is exact: np.std uses ddof = 0, so std over samples of x_s . a is ||a (X - mean)^T|| / sqrt(nsam).
Pure numpy, so that it can be checked without a GPU; ``fold`` is the kernel's formula in numpy.
"""
from __future__ import annotations

import numpy as np

QUAD, NORM = 0, 1          # fsnap_row_variance modes (_capi.UQ_QUAD, _capi.UQ_NORM)
METHODS = ("sam", "chol", "choleye", "svd", "loop", "fullcov")


def stdev_operator(method, cov=None, fit_sam=None):
    """(mode, M) of ``method``; None for a method the reference does not know (its ``else``: zeros).  Raises
    AssertionError when the method's input is missing and LinAlgError where the reference's factorisation does."""
    if method == "sam":
        assert fit_sam is not None
        X = np.asarray(fit_sam, dtype=np.float64)
        X = X.reshape(X.shape[0], -1)
        C = X - X.mean(axis=0)
        return NORM, np.ascontiguousarray(C.T / np.sqrt(X.shape[0]))
    if method not in METHODS:
        return None
    assert cov is not None
    cov = np.asarray(cov, dtype=np.float64)
    if method == "chol":
        return NORM, np.linalg.cholesky(cov)
    if method == "choleye":
        eigvals = np.linalg.eigvalsh(cov)
        return NORM, np.linalg.cholesky(cov + (abs(eigvals[0]) + 1e-14) * np.eye(cov.shape[0]))
    if method == "svd":
        u, s, _ = np.linalg.svd(cov, hermitian=True)
        return NORM, np.ascontiguousarray(u * np.sqrt(s))
    return QUAD, np.ascontiguousarray(cov)        # loop, fullcov


def fold(a, mode, M):
    """The kernel's per-row value in numpy: QUAD ((a M) * a).sum(1), NORM ((a M)^2).sum(1)."""
    a = np.asarray(a, dtype=np.float64)
    T = a @ M
    return (T * a).sum(axis=1) if mode == QUAD else (T * T).sum(axis=1)


def category_ids(labels):
    """Per-row labels -> (int32 ids, keys), keys numbered in first-seen order.  ``labels`` is one label per row (a list,
    array or anything iterable; a label may itself be a tuple), or a TUPLE of such per-row columns that together make
    the key, e.g. (groups, configs)."""
    if isinstance(labels, tuple):
        n = len(labels[0]) if labels else 0
        if any(len(col) != n for col in labels):
            raise ValueError("label columns differ in length")
        rows = list(zip(*labels))
    else:
        rows = [x.item() if isinstance(x, np.generic) else x for x in labels]
    ids = np.empty(len(rows), dtype=np.int32)
    pos = {}
    for i, key in enumerate(rows):
        ids[i] = pos.setdefault(key, len(pos))
    return ids, list(pos)


def strip_b0(values, ntypes, ncoeff, samples=False):
    """Undo ``Solver._offset``: drop the zero B0 it put in front of each type's ``ncoeff`` coefficients.  ``values`` is
    a fit (flat, or the column vector of several types) or, with ``samples``, one row per sample; values that have no
    B0 (ntypes * ncoeff entries per row) come back as they are (flat for a fit)."""
    v = np.asarray(values, dtype=np.float64)
    sam = bool(samples)
    rows = v.reshape(v.shape[0], -1) if sam else v.reshape(1, -1)
    if rows.shape[1] == ntypes * ncoeff:
        return rows if sam else rows[0]
    if rows.shape[1] != ntypes * (ncoeff + 1):
        raise ValueError(f"{rows.shape[1]} coefficients per row: neither {ntypes} x {ncoeff} nor {ntypes} x {ncoeff + 1}")
    out = rows.reshape(rows.shape[0], ntypes, ncoeff + 1)[:, :, 1:].reshape(rows.shape[0], ntypes * ncoeff)
    return out if sam else out[0]
