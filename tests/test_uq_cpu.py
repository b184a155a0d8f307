"""CPU: the host side of the predictive-variance pass (fitsnap_amd/solvers/uq.py) -- for every method of the reference's
Solver._compute_stdev (fitsnap3lib/solvers/solver.py:440-472) the matrix M folded by the kernel's formula gives the
reference formula's variance; the B0 stripping that undoes Solver._offset; the category helper; argument errors."""
import numpy as np
import pytest

from fitsnap_amd.solvers import uq


# the reference's formulas, restated (solver.py:440-472)
def ref_stdev(a, method, cov=None, fit_sam=None):
    if method == "sam":
        assert fit_sam is not None
        return np.std(fit_sam @ a.T, axis=0)
    if method == "chol":
        assert cov is not None
        return np.linalg.norm(a @ np.linalg.cholesky(cov), axis=1)
    if method == "choleye":
        assert cov is not None
        ev = np.linalg.eigvalsh(cov)
        return np.linalg.norm(a @ np.linalg.cholesky(cov + (abs(ev[0]) + 1e-14) * np.eye(cov.shape[0])), axis=1)
    if method == "svd":
        assert cov is not None
        u, s, vh = np.linalg.svd(cov, hermitian=True)
        return np.linalg.norm((a @ u) @ np.sqrt(np.diag(s)), axis=1)
    if method == "loop":
        assert cov is not None
        tmp = np.dot(a, cov)
        return np.array([np.sqrt(np.dot(tmp[i, :], a[i, :])) for i in range(a.shape[0])])
    if method == "fullcov":
        assert cov is not None
        return np.sqrt(np.diag((a @ cov) @ a.T))
    return np.zeros(a.shape[0])


def kernel_stdev(a, method, cov=None, fit_sam=None):
    op = uq.stdev_operator(method, cov, fit_sam)
    if op is None:
        return np.zeros(a.shape[0])
    mode, M = op
    with np.errstate(invalid="ignore"):
        return np.sqrt(uq.fold(a, mode, M))


def psd(K, seed, rank=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rank or K + 5, K))
    return X.T @ X / X.shape[0]


def close(x, ref, tol):
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(x))
    assert np.all(np.abs(x - ref)[fin] <= tol * np.abs(ref)[fin] + 1e-300)


@pytest.mark.parametrize("method", ["chol", "choleye", "svd", "loop", "fullcov"])
@pytest.mark.parametrize("K", [1, 7, 31, 64])
def test_every_cov_method_matches_reference_formula(method, K):
    a = np.random.default_rng(K).standard_normal((200, K))
    cov = psd(K, K + 1)
    close(kernel_stdev(a, method, cov), ref_stdev(a, method, cov), 1e-12)


def test_rank_deficient_cov():
    K = 20
    a = np.random.default_rng(0).standard_normal((100, K))
    cov = psd(K, 3, rank=8)
    cov[0, 0] -= 1e-12 * cov[0, 0] + 1e-9          # make sure it is not numerically PD either
    with pytest.raises(np.linalg.LinAlgError):
        uq.stdev_operator("chol", cov)
    with pytest.raises(np.linalg.LinAlgError):
        ref_stdev(a, "chol", cov)
    for method in ("choleye", "svd"):
        close(kernel_stdev(a, method, cov), ref_stdev(a, method, cov), 1e-10)
    # fullcov / loop: a tiny negative a^T C a gives NaN in both
    with np.errstate(invalid="ignore"):
        close(kernel_stdev(a, "fullcov", cov), ref_stdev(a, "fullcov", cov), 1e-6)


def test_merr_shaped_cov_with_zero_rows_and_columns():
    K = 12
    cov = np.zeros((K, K))
    keep = np.array([0, 2, 3, 7, 9, 11])
    cov[np.ix_(keep, keep)] = psd(len(keep), 5)
    a = np.random.default_rng(2).standard_normal((300, K))
    for method in ("svd", "loop", "fullcov", "choleye"):
        close(kernel_stdev(a, method, cov), ref_stdev(a, method, cov), 1e-10)
    with pytest.raises(np.linalg.LinAlgError):
        uq.stdev_operator("chol", cov)


@pytest.mark.parametrize("nsam", [1, 2, 20, 133])
def test_sam_is_exact(nsam):
    K = 31
    rng = np.random.default_rng(nsam)
    fit_sam = rng.standard_normal((nsam, K)) * 0.5 + rng.standard_normal(K)
    a = rng.standard_normal((500, K))
    mode, M = uq.stdev_operator("sam", None, fit_sam)
    assert mode == uq.NORM and M.shape == (K, nsam)
    P = fit_sam @ a.T
    ref = np.std(P, axis=0)
    got = np.sqrt(uq.fold(a, mode, M))
    # np.std subtracts the mean of the products AFTER forming them, so where the samples' products nearly agree the
    # reference formula itself carries an absolute error of a few eps max|p| (centring first does not)
    bar = 1e-13 * ref + 8 * np.finfo(float).eps * np.abs(P).max(axis=0)
    assert np.all(np.abs(got - ref) <= bar)
    assert np.median(np.abs(got - ref) / np.maximum(ref, 1e-300)) <= 1e-13


def test_missing_inputs_and_unknown_method():
    with pytest.raises(AssertionError):
        uq.stdev_operator("sam", np.eye(3), None)
    for method in ("chol", "choleye", "svd", "loop", "fullcov"):
        with pytest.raises(AssertionError):
            uq.stdev_operator(method, None, np.ones((3, 3)))
    assert uq.stdev_operator("nope", None, None) is None
    assert np.array_equal(kernel_stdev(np.ones((4, 3)), "nope"), np.zeros(4))


def test_strip_b0_one_type():
    fit = np.arange(1.0, 31.0)
    sam = np.arange(60.0).reshape(2, 30)
    fit_b0 = np.insert(fit, 0, 0)                               # Solver._offset, one type
    sam_b0 = np.insert(sam, 0, 0, axis=1)
    assert np.array_equal(uq.strip_b0(fit_b0, 1, 30), fit)
    assert np.array_equal(uq.strip_b0(sam_b0, 1, 30, samples=True), sam)
    assert np.array_equal(uq.strip_b0(fit, 1, 30), fit)          # no B0: as it is
    assert np.array_equal(uq.strip_b0(sam, 1, 30, samples=True), sam)


def test_strip_b0_several_types():
    ntypes, ncoeff = 3, 5
    fit = np.arange(1.0, 1 + ntypes * ncoeff)
    sam = np.arange(4.0 * ntypes * ncoeff).reshape(4, -1)

    def with_b0(rows):                                          # Solver._offset, several types
        blocks = rows.reshape(-1, ntypes, ncoeff)
        return np.pad(blocks, ((0, 0), (0, 0), (1, 0))).reshape(blocks.shape[0], ntypes * (ncoeff + 1))

    fit_b0 = with_b0(fit).reshape(-1, 1)
    sam_b0 = with_b0(sam)
    assert np.array_equal(uq.strip_b0(fit_b0, ntypes, ncoeff), fit)
    assert np.array_equal(uq.strip_b0(sam_b0, ntypes, ncoeff, samples=True), sam)
    with pytest.raises(ValueError):
        uq.strip_b0(np.ones(7), ntypes, ncoeff)


def test_category_ids():
    ids, keys = uq.category_ids(["b", "a", "b", "c", "a"])
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 0, 2, 1] and keys == ["b", "a", "c"]
    ids, keys = uq.category_ids((["g1", "g1", "g2", "g1"], ["c1", "c2", "c1", "c1"]))
    assert ids.tolist() == [0, 1, 2, 0] and keys == [("g1", "c1"), ("g1", "c2"), ("g2", "c1")]
    ids, keys = uq.category_ids(np.array([5, 3, 5]))
    assert ids.tolist() == [0, 1, 0] and keys == [5, 3]
    ids, keys = uq.category_ids([])
    assert ids.shape == (0,) and keys == []
    with pytest.raises(ValueError):
        uq.category_ids((["a", "b"], ["c"]))


def test_solver_has_the_methods():
    from fitsnap_amd.solvers.solver import Solver

    assert callable(getattr(Solver, "_compute_stdev")) and callable(getattr(Solver, "prediction_variance"))
    import inspect

    assert list(inspect.signature(Solver._compute_stdev).parameters) == ["self", "a", "method"]
    assert inspect.signature(Solver._compute_stdev).parameters["method"].default == "chol"
