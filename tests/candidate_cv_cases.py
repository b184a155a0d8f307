"""Cases, oracles and tolerances of the grouped K-fold cross-validation of weight candidates (tests/test_candidate_cv_cpu.py,
tests/test_gpu_candidate_cv.py).

Oracle R (rows): for each problem (p, f) the refit on the weighted rows without fold f -- the normal equations formed in long
double from the rows (64-bit mantissa: their own rounding is kappa 5e-20), Jacobi-scaled and solved by a long-double Cholesky;
columns no remaining row touches are removed (coefficient 0, the minimum-norm answer of ``lstsq``); ``alpha`` enters as the
sqrt(alpha) I rows of a ridge fit.  ``rows_lstsq`` is the same refit by ``numpy.linalg.lstsq`` on the weighted rows themselves;
the CPU tests tie the two together.  The residual sums are accumulated in long double.

Oracle H (host restatement): the formulas of ``fsnap_cv_candidates`` in plain numpy float64 from ``blocks_numpy`` blocks.

Tolerances are measured, not chosen: ``python tests/candidate_cv_cases.py`` prints the worst disagreement of oracle H from
oracle R over the sweep (and the Ta golden case), recorded below as MEASURED_*; the kernels get 10 x each (FMA contraction,
reduction order, the statistics summed per chunk on the matrix pipe instead of by the host BLAS).
  (a) MEASURED_BACKWARD: normwise backward error of beta on the exact Jacobi-scaled system of its problem
  (b) MEASURED_HELDOUT:  relative difference of the pooled held-out sum r^2 and sum |r| per (candidate, category)
  (c) MEASURED_FORWARD:  max |beta - beta_R| / max |beta_R| per problem
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import candidates_cv as ccv  # noqa: E402
from fitsnap_amd.solvers import lasso_path as lp  # noqa: E402
from fitsnap_amd.solvers import loco  # noqa: E402

LD = np.longdouble
EPS = np.finfo(np.float64).eps
PIVOT_TOL = 1e-10                                        # fsnap::LOCO_PIVOT_TOL

SWEEP_K = [1, 7, 31, 63, 64, 65, 128, 129, 143, 144]     # lane-ownership edges of a 64-lane wave, the LDS-size edge
SWEEP_CASES = [str(K) for K in SWEEP_K] + ["chunks"]     # "chunks": K = 31 with composite categories of 1 025 and 2 049 rows
SWEEP_F, SWEEP_C = 3, 4
SWEEP_P = 17                                             # batches 1, 16, 17 are prefixes: the 16-candidate tile edge of V2
BATCHES = (1, 16, 17)
PIVOT_FLOOR = 1e-6                                       # every sweep problem: oracle H's smallest scaled pivot is above this
ALPHA_FRACTIONS = (0.0, 1e-8)                            # alpha = fraction x mean diagonal of the base-weight total G

# Measured by ``python tests/candidate_cv_cases.py`` (oracle H against oracle R, worst over the cases named):
#   sweep: SWEEP_CASES x 17 candidates x 3 folds x both alphas;  Ta: the golden rows, 8 candidates x 5 folds, alpha 0 and 1e-8
#   (the Ta problems have smallest scaled pivots down to 3.3e-5, the sweep's stay above 3.0e-2: hence the two sets)
MEASURED_BACKWARD = 5.9e-16
MEASURED_HELDOUT = 2.5e-12
MEASURED_FORWARD = 1.2e-13
MEASURED_BACKWARD_TA = 9.3e-17
MEASURED_HELDOUT_TA = 1.5e-09
MEASURED_FORWARD_TA = 9.1e-11
BACKWARD_BAR = 10 * MEASURED_BACKWARD
HELDOUT_REL = 10 * MEASURED_HELDOUT
FORWARD_REL = 10 * MEASURED_FORWARD
BACKWARD_BAR_TA = 10 * MEASURED_BACKWARD_TA
HELDOUT_REL_TA = 10 * MEASURED_HELDOUT_TA
FORWARD_REL_TA = 10 * MEASURED_FORWARD_TA


def ga_scales(P, C, seed):
    """(P, C) scales drawn as the weight search draws them (``ga_candidates`` of tests/test_gpu_candidates.py): per group
    an energy weight 1e-4 ... 1e4 and force and stress ratios 1e-3 ... 1e3; the categories are (group, row type) pairs, even
    ones energy rows and odd ones force rows of group c // 2."""
    rng = np.random.default_rng(seed)
    ngroups = (C + 1) // 2
    S = np.empty((P, C))
    for p in range(P):
        ew = 10.0 ** rng.uniform(-4, 4, ngroups)
        fr = 10.0 ** rng.uniform(-3, 3, ngroups)
        rng.uniform(-3, 3, ngroups)                       # the stress ratios: drawn, no stress rows here
        for c in range(C):
            S[p, c] = ew[c // 2] * (fr[c // 2] if c % 2 else 1.0)
    return S


def composite_sizes(K, chunks=False):
    """Rows per composite category (F x C): about 3 K + 40 per fold; (fold 0, category 2) has no rows and category 3 lies
    wholly inside fold 2.  Every category that is present without a fold has more than K rows there, so the refit is
    determined whichever category a candidate weights up."""
    n = K + 13
    sizes = np.array([[(3 * K + 40) // 2, (3 * K + 41) // 2, 0, 0],
                      [n, n + 1, n + 1, 0],
                      [n, n, n, n]])
    if chunks:
        sizes[0, 0], sizes[1, 1] = 1025, 2049             # one row past one chunk, one row past two
    return sizes


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """(A, b, w0, composite category per row, K) of a sweep case: columns scaled over two decades, weights in [0.5, 2], rows in
    shuffled order, three rows without a category."""
    chunks = name == "chunks"
    K = 31 if chunks else int(name)
    sizes = composite_sizes(K, chunks)
    rng = np.random.default_rng(7000 + K + (500 if chunks else 0))
    ccat = np.concatenate([np.full(int(n), i, dtype=np.int32) for i, n in enumerate(sizes.ravel())] + [np.full(3, -1, dtype=np.int32)])
    rng.shuffle(ccat)
    m = len(ccat)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, K)
    A = rng.standard_normal((m, K)) * scale
    truth = rng.standard_normal(K) / scale
    b = A @ truth + 0.1 * rng.standard_normal(m)
    w0 = rng.uniform(0.5, 2.0, m)
    return np.ascontiguousarray(A), b, w0, ccat, K


def sweep_scales(name):
    return ga_scales(SWEEP_P, SWEEP_C, 90 + len(name) + sum(map(ord, name)))


def blocks_numpy(A, b, w, cat, ncat):
    """The packed per-category blocks [G | c | bb, sum wb, n] in numpy float64 (what fsnap_cat_normal_eq forms on the GPU, to
    rounding): ncat x (K^2 + K + 3).  cat < 0: the row takes no part."""
    K = A.shape[1]
    out = np.zeros((ncat, K * K + K + 3))
    for c in range(ncat):
        r = np.flatnonzero(cat == c)
        X, y = A[r] * w[r, None], b[r] * w[r]
        out[c, :K * K] = (X.T @ X).ravel()
        out[c, K * K:K * K + K] = X.T @ y
        out[c, K * K + K:] = (y @ y, y.sum(), len(r))
    return out


def blocks_ld(A, b, w, cat, ncat):
    """The same blocks accumulated in long double from the rows."""
    K = A.shape[1]
    out = np.zeros((ncat, K * K + K + 3), dtype=LD)
    for c in range(ncat):
        r = np.flatnonzero(cat == c)
        X = np.asarray(A[r], dtype=LD) * np.asarray(w[r], dtype=LD)[:, None]
        y = np.asarray(b[r], dtype=LD) * np.asarray(w[r], dtype=LD)
        out[c, :K * K] = (X.T @ X).ravel()
        out[c, K * K:K * K + K] = X.T @ y
        out[c, K * K + K:] = (y @ y, y.sum(), len(r))
    return out


def base_alpha(blocks, K, fraction):
    """fraction x the mean diagonal of the total G at the base weights."""
    G = blocks[:, :K * K].sum(axis=0).reshape(K, K)
    return float(fraction) * float(np.mean(np.diag(G)))


# ---- oracle R ---------------------------------------------------------------------------------------------------------
def chol_solve_ld(H, c):
    """x of H x = c by a long-double Cholesky (H symmetric positive definite)."""
    n = len(c)
    L, y = np.array(H, dtype=LD), np.array(c, dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for i in range(n - 1, -1, -1):
        y[i] /= L[i, i]
        y[:i] -= L[i, :i] * y[i]
    return y


def system_ld(bl, s, f, F, C, K):
    """(G, c) in long double of the refit of the scales s without fold f from the long-double blocks: the normal equations of
    the weighted rows that remain."""
    s2 = np.asarray(s, dtype=LD) ** 2
    acc = np.zeros(K * K + K, dtype=LD)
    for ff in range(F):
        if ff != f:
            for c in range(C):
                acc += s2[c] * bl[ff * C + c, :K * K + K]
    return acc[:K * K].reshape(K, K), acc[K * K:]


def refit_ld(bl, s, f, F, C, K, alpha):
    """Oracle R's coefficients of one problem (long double)."""
    G, c = system_ld(bl, s, f, F, C, K)
    live = np.diag(G) > 0
    beta = np.zeros(K, dtype=LD)
    if live.any():
        H = G[np.ix_(live, live)] + LD(alpha) * np.eye(int(live.sum()), dtype=LD)
        d = np.sqrt(np.diag(H))
        beta[live] = chol_solve_ld(H / d[:, None] / d[None, :], c[live] / d) / d
    return beta


def rows_lstsq(A, b, w0, ccat, s, f, C, alpha):
    """The same refit by ``numpy.linalg.lstsq`` (minimum norm) on the weighted rows without fold f, with sqrt(alpha) I rows."""
    keep = (ccat >= 0) & (ccat // C != f)
    wt = w0[keep] * np.asarray(s)[ccat[keep] % C]
    X, y = A[keep] * wt[:, None], b[keep] * wt
    K = A.shape[1]
    if alpha > 0:
        X, y = np.vstack([X, np.sqrt(alpha) * np.eye(K)]), np.concatenate([y, np.zeros(K)])
    return np.linalg.lstsq(X, y, rcond=None)[0]


def residual_sums_ld(A, b, w0, ccat, coef, F, C):
    """(P, F C, 4) sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2 of r = b - a . coef[p, fold of the row] per composite category,
    accumulated in long double."""
    P = coef.shape[0]
    out = np.zeros((P, F * C, 4))
    for cc in range(F * C):
        r_ = np.flatnonzero(ccat == cc)
        if not len(r_):
            continue
        Ar, br, wr = np.asarray(A[r_], dtype=LD), np.asarray(b[r_], dtype=LD), np.asarray(w0[r_], dtype=LD)
        for p in range(P):
            res = br - Ar @ np.asarray(coef[p, cc // C], dtype=LD)
            wres = wr * res
            out[p, cc] = (float(np.abs(res).sum()), float(res @ res), float(np.abs(wres).sum()), float(wres @ wres))
    return out


def oracle_r_from(A, b, w0, ccat, S, F, C, alpha):
    """(coef (P, F, K) long double, sums (P, F C, 4)) of oracle R."""
    K = A.shape[1]
    bl = blocks_ld(A, b, w0, ccat, F * C)
    coef = np.zeros((S.shape[0], F, K), dtype=LD)
    for p in range(S.shape[0]):
        for f in range(F):
            coef[p, f] = refit_ld(bl, S[p], f, F, C, K, alpha)
    return coef, residual_sums_ld(A, b, w0, ccat, coef, F, C), bl


@functools.lru_cache(maxsize=None)
def sweep_oracle(name, ialpha):
    """Oracle R of a sweep case at ALPHA_FRACTIONS[ialpha], computed once and shared: (alpha, coef float64, sums, counts,
    long-double blocks)."""
    A, b, w0, ccat, K = sweep_case(name)
    alpha = base_alpha(blocks_numpy(A, b, w0, ccat, SWEEP_F * SWEEP_C), K, ALPHA_FRACTIONS[ialpha])
    coef, sums, bl = oracle_r_from(A, b, w0, ccat, sweep_scales(name), SWEEP_F, SWEEP_C, alpha)
    counts = np.bincount(ccat[ccat >= 0], minlength=SWEEP_F * SWEEP_C)
    return alpha, np.asarray(coef, dtype=np.float64), sums, counts, bl


# ---- oracle H ---------------------------------------------------------------------------------------------------------
def host_cv(blocks, S, F, C, K, alpha):
    """``fsnap_cv_candidates`` restated in numpy float64: (coef (P, F, K), info (P, F, 4))."""
    blocks = np.asarray(blocks, dtype=np.float64).reshape(F, C, -1)
    total = blocks[0].copy()
    for f in range(1, F):
        total = total + blocks[f]
    P = S.shape[0]
    coef = np.zeros((P, F, K))
    info = np.zeros((P, F, 4))
    KK = K * K
    for p in range(P):
        s2 = S[p] * S[p]
        for f in range(F):
            acc, tp = np.zeros(KK + K + 3), np.zeros(K)
            for c in range(C):
                acc = acc + s2[c] * (total[c] - blocks[f, c])
                tp = tp + s2[c] * np.diag(total[c, :KK].reshape(K, K))
            Qm, qv = acc[:KK].reshape(K, K), acc[KK:KK + K]
            qjj = np.diag(Qm)
            live = ~((tp == 0.0) | (qjj <= PIVOT_TOL * tp))
            k = int(live.sum())
            status, minpiv = 0, np.inf
            if k:
                H = Qm[np.ix_(live, live)] + alpha * np.eye(k)
                d = np.sqrt(np.diag(H))
                Hs = H / d[:, None] / d[None, :]
                try:
                    L = np.linalg.cholesky(Hs)
                    minpiv = float(np.min(np.diag(L)) ** 2)
                except np.linalg.LinAlgError:
                    minpiv, status = 0.0, 1
                if status == 0 and not minpiv > PIVOT_TOL:
                    status = 1
                if status == 0:
                    y = np.linalg.solve(L, qv[live] / d)
                    coef[p, f, live] = np.linalg.solve(L.T, y) / d
            if status:
                coef[p, f] = np.nan
            info[p, f] = (status, minpiv, k, acc[KK + K + 2])
    return coef, info


def host_sums(A, b, w0, ccat, coef, F, C):
    """``fsnap_cv_candidate_rows`` restated in numpy float64: (P, F C, 4)."""
    P = coef.shape[0]
    out = np.zeros((P, F * C, 4))
    for cc in range(F * C):
        r_ = np.flatnonzero(ccat == cc)
        for p in range(P):
            res = b[r_] - A[r_] @ coef[p, cc // C]
            wres = w0[r_] * res
            out[p, cc] = (np.abs(res).sum(), (res * res).sum(), np.abs(wres).sum(), (wres * wres).sum())
    return out


# ---- the three measured quantities --------------------------------------------------------------------------------------
def backward_error(H, c, beta):
    """Normwise backward error of beta as a solution of H beta = c after Jacobi scaling (the ``backward_error`` of
    tests/test_gpu_candidates.py)."""
    d = np.sqrt(np.diag(H))
    Hs, xs, cs = H / d[:, None] / d[None, :], beta * d, c / d
    return float(np.linalg.norm(Hs @ xs - cs) / (np.linalg.norm(Hs, 2) * np.linalg.norm(xs) + np.linalg.norm(cs)))


def worst_backward(bl, S, F, C, K, alpha, coef):
    """(a): the worst backward error of coef[p, f] on the exact system of (p, f) (long-double blocks, live columns)."""
    worst = 0.0
    for p in range(coef.shape[0]):
        for f in range(F):
            G, c = system_ld(bl, S[p], f, F, C, K)
            live = np.diag(G) > 0
            if not live.any():
                continue
            H = np.asarray(G[np.ix_(live, live)], dtype=np.float64) + alpha * np.eye(int(live.sum()))
            worst = max(worst, backward_error(H, np.asarray(c[live], dtype=np.float64), coef[p, f][live]))
    return worst


def worst_heldout(sums, ref, counts, S, F):
    """(b): the worst relative difference of the pooled sum |r| and sum r^2 per (candidate, category) with rows."""
    got, want = ccv.pool_heldout(sums, counts, S, F), ccv.pool_heldout(ref, counts, S, F)
    has = want[:, :, 0] > 0
    return float(np.max(np.abs(got[:, :, 1:3] - want[:, :, 1:3])[has] / want[:, :, 1:3][has]))


def worst_forward(coef, ref):
    """(c): the worst max |beta - beta_R| / max |beta_R| over the problems."""
    num = np.max(np.abs(coef - ref), axis=-1)
    den = np.maximum(np.max(np.abs(ref), axis=-1), 1e-300)
    return float(np.max(num / den))


# ---- the Ta golden case ----------------------------------------------------------------------------------------------
TA_ROW_TYPE = ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178
TA_P, TA_F = 8, 5
TA_ALPHAS = {"SVD": 0.0, "RIDGE": 1e-8}


def ta_labels(ta_fits):
    """fs_dict of the golden rows with ``Configs = c{i // 7}``, as the LOCO tests label them."""
    m = len(TA_ROW_TYPE)
    return {"Groups": [str(g) for g in ta_fits["ea_groups"]], "Testing": ta_fits["testing_mask"].tolist(), "Row_Type": TA_ROW_TYPE,
            "Configs": [f"c{i // 7}" for i in range(m)]}


def ta_candidates(groups, P, seed):
    """``ga_candidates`` of tests/test_gpu_candidates.py."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(P):
        ew = 10.0 ** rng.uniform(-4, 4, len(groups))
        fr = 10.0 ** rng.uniform(-3, 3, len(groups))
        sr = 10.0 ** rng.uniform(-3, 3, len(groups))
        out.append({g: {"eweight": ew[i], "fweight": ew[i] * fr[i], "vweight": ew[i] * sr[i]} for i, g in enumerate(groups)})
    return out


def ta_layout(fs, seed=0):
    """(category per row, keys, composite category per row, fold_of_unit, S) of the golden case without a GPU: the categories
    of ``CandidateFits``, folds from ``deal_folds``."""
    from fitsnap_amd.solvers.candidates import ROW_TYPE_WEIGHT, CandidateFits

    m = len(fs["Testing"])
    cat, keys = CandidateFits._categories(fs, m)
    train = ~np.asarray(fs["Testing"], dtype=bool)
    _, _, units = loco.unit_index(fs["Configs"], train)
    fold_of_unit, F = lp.deal_folds(units, TA_F, seed)
    fold = lp.row_categories(fs["Configs"], train, fold_of_unit, None, 1)
    C = len(keys)
    ccat = np.where(fold >= 0, fold * C + cat, -1).astype(np.int32)
    cands = ta_candidates(sorted(set(fs["Groups"])), TA_P, seed=11)
    S = np.array([[float(t[g][ROW_TYPE_WEIGHT[rt]]) for (g, _, rt) in keys] for t in cands])
    return cat, keys, ccat, fold_of_unit, S


@functools.lru_cache(maxsize=None)
def ta_oracle(name):
    """Oracle R of the golden case for solver ``name``: (coef float64, sums (P, F C, 4), counts, S, keys, ccat, blocks)."""
    golden = os.path.join(ROOT, "tests", "golden")
    z, fits = np.load(os.path.join(golden, "ta_abw.npz")), dict(np.load(os.path.join(golden, "ta_reference_fits.npz")))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    w = np.ones(len(b))                                   # the search's weights are absolute: the base weight is 1
    _, keys, ccat, _, S = ta_layout(ta_labels(fits))
    C = len(keys)
    coef, sums, bl = oracle_r_from(A, b, w, ccat, S, TA_F, C, TA_ALPHAS[name])
    counts = np.bincount(ccat[ccat >= 0], minlength=TA_F * C)
    return np.asarray(coef, dtype=np.float64), sums, counts, S, keys, ccat, bl


def measure():
    """Prints what the MEASURED_* constants record."""
    wa = wb = wc = 0.0
    minpiv = np.inf
    for name in SWEEP_CASES:
        A, b, w0, ccat, K = sweep_case(name)
        S = sweep_scales(name)
        blocks = blocks_numpy(A, b, w0, ccat, SWEEP_F * SWEEP_C)
        for ia in range(len(ALPHA_FRACTIONS)):
            alpha, ref, ref_sums, counts, bl = sweep_oracle(name, ia)
            coef, info = host_cv(blocks, S, SWEEP_F, SWEEP_C, K, alpha)
            assert not info[:, :, 0].any()
            ka = worst_backward(bl, S, SWEEP_F, SWEEP_C, K, alpha, coef)
            kb = worst_heldout(host_sums(A, b, w0, ccat, coef, SWEEP_F, SWEEP_C), ref_sums, counts, S, SWEEP_F)
            kc = worst_forward(coef, ref)
            print(f"{name:>6s} alpha {alpha:.2e}  backward {ka:.2e}  held-out {kb:.2e}  forward {kc:.2e}  "
                  f"min pivot {info[:, :, 1].min():.2e}", flush=True)
            wa, wb, wc, minpiv = max(wa, ka), max(wb, kb), max(wc, kc), min(minpiv, info[:, :, 1].min())
    print(f"MEASURED_BACKWARD = {wa:.1e}  MEASURED_HELDOUT = {wb:.1e}  MEASURED_FORWARD = {wc:.1e}  (min pivot {minpiv:.1e})")
    golden = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(golden, "ta_abw.npz"))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    w = np.ones(len(b))
    ta = tb = tc = 0.0
    for name in TA_ALPHAS:
        ref, ref_sums, counts, S, keys, ccat, bl = ta_oracle(name)
        C, K = len(keys), A.shape[1]
        coef, info = host_cv(blocks_numpy(A, b, w, ccat, TA_F * C), S, TA_F, C, K, TA_ALPHAS[name])
        assert not info[:, :, 0].any()
        ka = worst_backward(bl, S, TA_F, C, K, TA_ALPHAS[name], coef)
        kb = worst_heldout(host_sums(A, b, w, ccat, coef, TA_F, C), ref_sums, counts, S, TA_F)
        kc = worst_forward(coef, ref)
        print(f"Ta {name:5s} backward {ka:.2e}  held-out {kb:.2e}  forward {kc:.2e}  min pivot {info[:, :, 1].min():.2e}", flush=True)
        ta, tb, tc = max(ta, ka), max(tb, kb), max(tc, kc)
    print(f"MEASURED_BACKWARD_TA = {ta:.1e}  MEASURED_HELDOUT_TA = {tb:.1e}  MEASURED_FORWARD_TA = {tc:.1e}")


if __name__ == "__main__":
    measure()
