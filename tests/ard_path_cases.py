"""Cases, oracles and tolerances of the grouped K-fold ARD threshold path (tests/test_ard_path_cpu.py,
tests/test_gpu_ard_path.py).

Oracle A: ``ard_path.ard_path_host`` -- ``ARD._ard_loop`` (``pinvh``) on the fold blocks downdated in numpy.  Oracle B:
``ard_numpy`` in float64 -- the iteration as the kernel runs it (right-looking Cholesky of the equilibrated matrix of the kept
columns, its inverse, column sums), in numpy without FMA.  Oracle C: the same function in ``np.longdouble``, with the trace of
every decision.  Oracle D: scikit-learn's ``ARDRegression(fit_intercept=False, **hyper)`` on the weighted rows without the fold
(what the reference's class calls).

Decision margins are a CONDITION of a case, not a measurement: along oracle C's trace every updated lambda_j has
|lambda_j / threshold_lambda - 1| >= MARGIN and every stopping test |sum |d coef| / tol - 1| >= MARGIN (``oracle_c``, asserted
for every problem the tests use).  Under it support, iteration count and status must be EQUAL between the kernel, oracle A and
oracle C: the routes differ by 1e-15 ... 1e-9, MARGIN is 1e-6.

Tolerances: 10 x what oracle B differs from oracle A by over the sweep (``python tests/ard_path_cases.py`` prints the
MEASURED_* constants recorded below); against oracle D, 10 x what oracle A itself differs from D by.
"""
import functools
import os
import sys

import numpy as np
import sklearn.linear_model  # noqa: F401  (before the first host solve: the BLAS limiter looks its libraries up once)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fitsnap_amd.solvers import ard_path as ap  # noqa: E402
from fitsnap_amd.solvers import lasso_path as lp  # noqa: E402
from lasso_path_cases import blocks_numpy, fold_rows, heldout_ld, heldout_numpy, sweep_case  # noqa: E402,F401

LD = np.longdouble
EPS = np.finfo(np.float64).eps

SWEEP_K = [1, 7, 31, 63, 64, 65, 128, 129, 143, 144]     # wave-ownership edges of 64-lane waves, the LDS-size edge
SWEEP_F, SWEEP_Q = 3, 4
LOGCUTS = [0.3, 1.0, 2.0, 3.0]
TOL, MAX_ITER = 1e-3, 1000                                # ARD.TOL, ARD.MAX_ITER
MARGIN = 1e-6

# Measured by ``python tests/ard_path_cases.py`` over SWEEP_K x (F + 1) x Q problems (logcut in LOGCUTS, tol = 1e-3), oracle B
# against oracle A:
#   MEASURED_COEF     max |d (beta_B - beta_A)| / max |d beta_A|, d = sqrt(diag Qm)
#   MEASURED_LAMBDA   max |lambda_B / lambda_A - 1|
#   MEASURED_ALPHA    |alpha_B / alpha_A - 1|
#   MEASURED_DELTA    |delta_B - delta_A| / sum |beta_A|          (delta: the last sum |coef_old - coef|)
#   MEASURED_PIVOT    |pivot_B / pivot_A - 1|                     (the smallest Cholesky pivot; A's comes from LAPACK)
# and the numpy float64 three-term held-out formula against the row-wise long-double sum, relative: MEASURED_HELDOUT.
# The kernel is allowed 10 x each (FMA contraction, reduction order).
MEASURED_COEF = 6.8e-15
MEASURED_LAMBDA = 1.5e-10
MEASURED_ALPHA = 5.4e-12
MEASURED_DELTA = 6.0e-15
MEASURED_PIVOT = 1.8e-15
MEASURED_HELDOUT = 4.0e-12
# Oracle A against oracle D (scikit-learn on the rows), the scaled coefficient difference: sweep_case(31), every fold and
# LOGCUTS; the golden Ta rows, the groups TA_GROUPS left out and none, TA_LOGCUTS.
MEASURED_D_SWEEP = 1.2e-13
MEASURED_D_TA = 8.5e-06
# The three-term held-out formula against the row-wise long-double sum on the Ta rows (the same problems; columns over 15
# decades cancel harder than the sweep's two).
MEASURED_HELDOUT_TA = 8.8e-10
COEF_REL, LAMBDA_REL, ALPHA_REL = 10 * MEASURED_COEF, 10 * MEASURED_LAMBDA, 10 * MEASURED_ALPHA
DELTA_REL, PIVOT_REL, HELDOUT_REL = 10 * MEASURED_DELTA, 10 * MEASURED_PIVOT, 10 * MEASURED_HELDOUT
D_SWEEP_REL, D_TA_REL, HELDOUT_TA_REL = 10 * MEASURED_D_SWEEP, 10 * MEASURED_D_TA, 10 * MEASURED_HELDOUT_TA
# the host route against the iteration in extended precision on the Ta rows (columns over 15 decades): what solvers/ard.py
# documents for the equilibrated inverse, 1e-6
TA_C_REL = 1e-6
TA_LOGCUTS = [0.0, 0.3, 1.0, 2.0]
TA_GROUPS = 3                                             # leave-one-group-out over the first three groups (sorted names)


def settings(logcuts=LOGCUTS, scap=1e-3, scai=1e-3):
    return [{"logcut": float(x), "scap": scap, "scai": scai} for x in logcuts]


def hypers(blocks, K, grid, direct=False, nsub=1):
    """(hyper, run) of every (fold, setting) from the blocks."""
    folds, total = lp.sum_blocks(blocks, nsub)
    return ap.fold_hypers(folds, total, K, grid, direct)


def scaled_diff(Qm, beta, ref):
    """max |d (beta - ref)| / max |d ref|, d = sqrt(diag Qm); 0 when both vanish."""
    d = np.sqrt(np.maximum(np.diag(np.asarray(Qm, dtype=np.float64)), 0.0))
    den = float(np.max(np.abs(d * ref))) if len(ref) else 0.0
    num = float(np.max(np.abs(d * (np.asarray(beta, dtype=np.float64) - ref)))) if len(ref) else 0.0
    return num / den if den > 0 else num


def cholesky_lower(W):
    """Right-looking Cholesky of a symmetric matrix (its lower triangle), column by column as the kernel runs it: (L, pivots).
    ArithmeticError at a pivot that is not positive."""
    A = np.array(W)
    k = A.shape[0]
    piv = np.empty(k, dtype=A.dtype)
    for j in range(k):
        piv[j] = A[j, j]
        if not piv[j] > 0:
            raise ArithmeticError(float(piv[j]))
        ljj = np.sqrt(piv[j])
        col = A[j + 1:, j] / ljj
        A[j, j], A[j + 1:, j] = ljj, col
        A[j + 1:, j + 1:] -= np.outer(col, col)
    return np.tril(A), piv


def inverse_lower(L):
    """M = L^-1 from the last column: M_jj = 1 / L_jj, M[j + 1:, j] = -(M[j + 1:, j + 1:] L[j + 1:, j]) M_jj."""
    k = L.shape[0]
    M = np.zeros_like(L)
    for j in range(k - 1, -1, -1):
        M[j, j] = 1 / L[j, j]
        if j + 1 < k:
            M[j + 1:, j] = -(M[j + 1:, j + 1:] @ L[j + 1:, j]) * M[j, j]
    return M


def ard_numpy(Qm, qv, y2, n, dead, hyper, max_iter=MAX_ITER, tol=TOL, dtype=np.float64, trace=None):
    """The iteration of ``fsnap_ard_path`` on one downdated system in ``dtype``.  Returns (coef, lambda, info (6)); with a
    ``trace`` list, appends per iteration (lambda ratios lambda_j / threshold of the updated columns, sum |d coef| / tol or
    None in the first iteration)."""
    t = dtype
    Qm, qv = np.asarray(Qm, dtype=t), np.asarray(qv, dtype=t)
    y2, n, tol = t(y2), t(n), t(tol)
    a1, a2, l1, l2, thr, alpha = (t(x) for x in hyper)
    K = len(qv)
    live = ~np.asarray(dead, dtype=bool)
    d = np.ones(K, dtype=t)
    d[live] = np.sqrt(np.diag(Qm)[live])
    coef, cold, lam, keep = np.zeros(K, dtype=t), np.zeros(K, dtype=t), np.ones(K, dtype=t), live.copy()
    state = {"pivot": np.inf, "delta": np.inf}

    def solve(keep, alpha):
        dk = d[keep]
        W = alpha * (Qm[np.ix_(keep, keep)] / np.outer(dk, dk))
        W[np.diag_indices_from(W)] = lam[keep] / (dk * dk) + np.diag(W)
        L, piv = cholesky_lower(W)
        state["pivot"] = min(state["pivot"], float(piv.min()))
        M = inverse_lower(L)
        z = M @ (qv[keep] / dk)
        return M.T @ z, np.sum(M * M, axis=0), dk

    iters, status = 0, 2 if keep.any() else 0
    try:
        for it in range(max_iter if keep.any() else 0):
            iters = it + 1
            cs, sig, dk = solve(keep, alpha)
            ck = alpha * (cs / dk)
            coef[keep] = ck
            gamma = 1 - lam[keep] * (sig / (dk * dk))
            sse = max(y2 - 2 * (ck @ qv[keep]) + ck @ (Qm[np.ix_(keep, keep)] @ ck), t(0))
            new = (gamma + 2 * l1) / (ck * ck + 2 * l2)
            alpha = (n - gamma.sum() + 2 * a1) / (sse + 2 * a2)
            if not (np.all(np.isfinite(new)) and np.isfinite(alpha)):
                raise ArithmeticError("lambda")
            lam[keep] = new
            keep = (lam < thr) & live
            coef[~keep] = 0
            state["delta"] = float(np.sum(np.abs(cold - coef)))
            if trace is not None:
                trace.append((np.asarray(new / thr, dtype=np.float64), float(np.sum(np.abs(cold - coef)) / tol) if it > 0 else None))
            if it > 0 and np.sum(np.abs(cold - coef)) < tol:
                status = 0
                break
            cold = coef.copy()
            if not keep.any():
                status = 0
                break
        if keep.any():
            cs, _, dk = solve(keep, alpha)
            coef[keep] = alpha * (cs / dk)
    except ArithmeticError as failure:
        if isinstance(failure.args[0], float):                            # the pivot that failed counts among the pivots
            state["pivot"] = min(state["pivot"], failure.args[0])
        return np.full(K, np.nan), np.full(K, np.nan), np.array([iters, 0, float(alpha), state["delta"], state["pivot"], 1.0])
    info = np.array([iters, keep.sum(), float(alpha), state["delta"], state["pivot"], status], dtype=np.float64)
    return np.asarray(coef, dtype=np.float64), np.asarray(lam, dtype=np.float64), info


def margins(trace):
    """(smallest |lambda_j / threshold - 1|, smallest |sum |d coef| / tol - 1|) along a trace (inf where there is none)."""
    m_thr = min((float(np.min(np.abs(r - 1.0))) for r, _ in trace if len(r)), default=np.inf)
    m_stop = min((abs(s - 1.0) for _, s in trace if s is not None), default=np.inf)
    return m_thr, m_stop


def oracle_c(blocks, K, hyper, run=None, max_iter=MAX_ITER, tol=TOL, nsub=1, problems=None):
    """Oracle C over the problems ((f, q) pairs; default all): {(f, q): (coef, lambda, info)}; every problem is ADMITTED --
    asserted to keep the decision margins -- on the way."""
    folds, total = lp.sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], hyper.shape[1]
    out = {}
    systems = {}
    for f, q in (problems if problems is not None else [(f, q) for f in range(F + 1) for q in range(Q)]):
        if run is not None and not run[f, q]:
            continue
        if f not in systems:
            systems[f] = lp.downdated(folds, total, f, K)
        Qm, qv, y2, n, dead = systems[f]
        trace = []
        out[(f, q)] = ard_numpy(Qm, qv, y2, n, dead, hyper[f, q], max_iter, tol, dtype=LD, trace=trace)
        m_thr, m_stop = margins(trace)
        assert m_thr >= MARGIN and m_stop >= MARGIN, (K, f, q, "decision margins", m_thr, m_stop)
    return out


@functools.lru_cache(maxsize=None)
def sweep_problem(K):
    """(A, b, w, fold, blocks (numpy), grid, hyper, run) of the geometry sweep at K."""
    A, b, w, fold, _ = sweep_case(K)
    blocks = blocks_numpy(A, b, w, fold, SWEEP_F)
    grid = settings()
    hyper, run = hypers(blocks, K, grid)
    return A, b, w, fold, blocks, grid, hyper, run


def sklearn_refit(A, b, w, train, hyper, tol=TOL, max_iter=MAX_ITER):
    """Oracle D on the weighted rows ``train`` (boolean mask): (coef, lambda, n_iter)."""
    from sklearn.linear_model import ARDRegression

    X, y = A[train] * w[train, None], b[train] * w[train]
    a1, a2, l1, l2, thr, _ = (float(x) for x in hyper)
    m = ARDRegression(fit_intercept=False, alpha_1=a1, alpha_2=a2, lambda_1=l1, lambda_2=l2, threshold_lambda=thr, tol=tol,
                      max_iter=max_iter).fit(X, y)
    return m.coef_.copy(), m.lambda_.copy(), int(m.n_iter_)


def compare(K, blocks, hyper, out, ref, run=None, nsub=1, rel=None, where=""):
    """Equal support, iterations and status of ``out`` (coef, lambda, info, heldout) against ``ref`` (the same tuple), and the
    values within ``rel`` (default: the measured bars) -- the worst figures are returned."""
    rel = rel or dict(coef=COEF_REL, lam=LAMBDA_REL, alpha=ALPHA_REL, delta=DELTA_REL, pivot=PIVOT_REL, held=HELDOUT_REL)
    folds, total = lp.sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], hyper.shape[1]
    coef, lam, info, held = out
    rc, rl, ri, rh = ref
    worst = dict.fromkeys(rel, 0.0)
    for f in range(F + 1):
        Qm, qv, y2, n, dead = lp.downdated(folds, total, f, K)
        for q in range(Q):
            if run is not None and not run[f, q]:
                continue
            at = (where, K, f, q)
            assert info[f, q, 5] == ri[f, q, 5] and info[f, q, 0] == ri[f, q, 0] and info[f, q, 1] == ri[f, q, 1], (at, info[f, q], ri[f, q])
            if ri[f, q, 5] == 1:
                assert np.all(np.isnan(coef[f, q])) and np.all(np.isnan(lam[f, q])), at
                continue
            assert np.array_equal(coef[f, q] != 0, rc[f, q] != 0) and np.all(coef[f, q][dead] == 0), at
            assert np.array_equal(lam[f, q] < hyper[f, q, 4], rl[f, q] < hyper[f, q, 4]), at
            fig = dict(coef=scaled_diff(Qm, coef[f, q], rc[f, q]), lam=float(np.max(np.abs(lam[f, q] / rl[f, q] - 1.0))) if K else 0.0,
                       alpha=abs(info[f, q, 2] / ri[f, q, 2] - 1.0))
            if np.isfinite(ri[f, q, 3]):
                s = float(np.sum(np.abs(rc[f, q])))
                fig["delta"] = abs(info[f, q, 3] - ri[f, q, 3]) / s if s > 0 else abs(info[f, q, 3] - ri[f, q, 3])
            else:
                assert info[f, q, 3] == ri[f, q, 3], at
            if np.isfinite(ri[f, q, 4]):
                fig["pivot"] = abs(info[f, q, 4] / ri[f, q, 4] - 1.0)
            else:
                assert info[f, q, 4] == ri[f, q, 4], at
            if f < F:
                assert held[f, q, 0] == rh[f, q, 0] and held[f, q, 2] == rh[f, q, 2], at
                if rh[f, q, 1] != 0:
                    fig["held"] = abs(held[f, q, 1] / rh[f, q, 1] - 1.0)
            for key, v in fig.items():
                assert v <= rel[key], (at, key, v, rel[key])
                worst[key] = max(worst[key], v)
    return worst


def ta_rows():
    """The golden Ta rows and their group of every row: (A, b, w, fold id per row by sorted group name, group names)."""
    golden = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(golden, "ta_abw.npz"))
    groups = np.load(os.path.join(golden, "ta_reference_fits.npz"))["ea_groups"]
    names = sorted(set(groups.tolist()))
    fold = np.array([names.index(g) for g in groups])
    return np.ascontiguousarray(d["A"]), np.ascontiguousarray(d["b"]), np.ascontiguousarray(d["w"]), fold, names


@functools.lru_cache(maxsize=None)
def ta_problem():
    """(A, b, w, fold, names, blocks (numpy), grid, hyper, run, problems) of the Ta case: every group a fold; the problems the
    tests look at are the first TA_GROUPS folds and the fit on all rows, at TA_LOGCUTS."""
    A, b, w, fold, names = ta_rows()
    F = len(names)
    blocks = blocks_numpy(A, b, w, fold, F)
    grid = settings(TA_LOGCUTS)
    hyper, run = hypers(blocks, A.shape[1], grid)
    problems = [(f, q) for f in list(range(TA_GROUPS)) + [F] for q in range(len(grid))]
    return A, b, w, fold, names, blocks, grid, hyper, run, problems


def measure():
    """Prints what the MEASURED_* constants record."""
    worst = dict(coef=0.0, lam=0.0, alpha=0.0, delta=0.0, pivot=0.0, held=0.0)
    loose = dict.fromkeys(worst, np.inf)
    for K in SWEEP_K:
        A, b, w, fold, blocks, grid, hyper, run = sweep_problem(K)
        host = ap.ard_path_host(blocks, K, hyper, MAX_ITER, TOL)
        oracle_c(blocks, K, hyper, run)                                   # admits every problem
        folds, total = lp.sum_blocks(blocks)
        B = (np.zeros_like(host[0]), np.zeros_like(host[1]), np.zeros_like(host[2]), host[3].copy())
        kh = 0.0
        for f in range(SWEEP_F + 1):
            Qm, qv, y2, n, dead = lp.downdated(folds, total, f, K)
            for q in range(len(grid)):
                B[0][f, q], B[1][f, q], B[2][f, q] = ard_numpy(Qm, qv, y2, n, dead, hyper[f, q])
                if f < SWEEP_F:
                    B[3][f, q, 1] = heldout_numpy(folds[f], K, B[0][f, q])
                    ref = heldout_ld(A, b, w, np.flatnonzero(fold == f), host[0][f, q])
                    kh = max(kh, abs(heldout_numpy(folds[f], K, host[0][f, q]) - ref) / ref)
        fig = compare(K, blocks, hyper, B, host, rel=loose, where="measure")
        fig["held"] = kh
        print(f"K = {K:3d}  B vs A: coef {fig['coef']:.2e}  lambda {fig['lam']:.2e}  alpha {fig['alpha']:.2e}  delta {fig['delta']:.2e}  "
              f"pivot {fig['pivot']:.2e}   three-term vs long double {kh:.2e}   iterations {int(host[2][:, :, 0].min())} ... "
              f"{int(host[2][:, :, 0].max())}  kept {int(host[2][:, :, 1].min())} ... {int(host[2][:, :, 1].max())}", flush=True)
        for key in worst:
            worst[key] = max(worst[key], fig[key])
    print("MEASURED_COEF = {coef:.1e}  MEASURED_LAMBDA = {lam:.1e}  MEASURED_ALPHA = {alpha:.1e}  MEASURED_DELTA = {delta:.1e}  "
          "MEASURED_PIVOT = {pivot:.1e}  MEASURED_HELDOUT = {held:.1e}".format(**worst))
    # oracle A against oracle D
    A, b, w, fold, blocks, grid, hyper, run = sweep_problem(31)
    host = ap.ard_path_host(blocks, 31, hyper, MAX_ITER, TOL)
    folds, total = lp.sum_blocks(blocks)
    d_sweep = 0.0
    for f in range(SWEEP_F + 1):
        Qm = lp.downdated(folds, total, f, 31)[0]
        for q in range(len(grid)):
            ref, _, nit = sklearn_refit(A, b, w, fold != f, hyper[f, q])
            assert np.array_equal(ref != 0, host[0][f, q] != 0) and nit == host[2][f, q, 0], (f, q)
            d_sweep = max(d_sweep, scaled_diff(Qm, host[0][f, q], ref))
    A, b, w, fold, names, blocks, grid, hyper, run, problems = ta_problem()
    K = A.shape[1]
    host = ap.ard_path_host(blocks, K, hyper, MAX_ITER, TOL)
    C = oracle_c(blocks, K, hyper, run, problems=problems)
    folds, total = lp.sum_blocks(blocks)
    d_ta = c_ta = h_ta = 0.0
    for f, q in problems:
        Qm = lp.downdated(folds, total, f, K)[0]
        ref, _, nit = sklearn_refit(A, b, w, fold != f, hyper[f, q])
        same = np.array_equal(ref != 0, host[0][f, q] != 0) and nit == host[2][f, q, 0]
        d = scaled_diff(Qm, host[0][f, q], ref)
        c = scaled_diff(Qm, host[0][f, q], C[(f, q)][0])
        print(f"Ta  fold {f:2d} ({names[f] if f < len(names) else 'none'})  logcut {grid[q]['logcut']}: A vs D {d:.2e} "
              f"(support and iterations equal: {same})  A vs C {c:.2e}  iterations {int(host[2][f, q, 0])}  kept {int(host[2][f, q, 1])}",
              flush=True)
        d_ta, c_ta = max(d_ta, d), max(c_ta, c)
        if f < len(names):
            true = heldout_ld(A, b, w, np.flatnonzero(fold == f), host[0][f, q])
            h_ta = max(h_ta, abs(heldout_numpy(folds[f], K, host[0][f, q]) - true) / true)
    print(f"MEASURED_D_SWEEP = {d_sweep:.1e}  MEASURED_D_TA = {d_ta:.1e}  MEASURED_HELDOUT_TA = {h_ta:.1e}   (A vs C on Ta: {c_ta:.1e}, allowed TA_C_REL = {TA_C_REL:.0e})")


if __name__ == "__main__":
    measure()
