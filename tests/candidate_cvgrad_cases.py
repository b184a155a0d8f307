"""Cases, oracles and tolerances of the gradient of the cross-validated cost over the group weights
(tests/test_candidate_cvgrad_cpu.py, tests/test_gpu_candidate_cvgrad.py).

Oracle R: long double throughout.  The blocks are accumulated from the rows (``cc.blocks_ld``), every refit is the long-double
Cholesky solve of ``cc.refit_ld``, the held-out sums come from the rows (``heldout_ld``), and the adjoint formulas of
solvers/candidates_cv_grad.py -- g, lambda, D, dJ/dS, dJ/dlog alpha -- are evaluated on them in long double.

Oracle H: ``candidates_cv_grad.host_gradient``, the float64 numpy restatement, on ``cc.blocks_numpy`` blocks with the refits of
``cc.host_cv``.

Error measures, safe against cancellation (every scale is taken from oracle R):
  g        |g - g_R| / sg,          sg[p, f, k]  = 2 sum_c |omega| (|B.G| |beta| + |B.r|)_k
  lambda   max_k |lam - lam_R| / max_k |lam_R| per problem (lambda = H^-1 g: a forward error, as ``cc.worst_forward``)
  grad_S   |grad_S - ref| / scale,  scale[p, c]  = 2 |S| sum_f |lam| . (|R.r| + |R.G| |beta|)
  alpha    |gla - ref| / sa,        sa[p]        = alpha sum_f |lam| . |beta|          (alpha = 0: gla must be exactly 0)
  invariant |sum_c S dJ/dS + 2 dJ/dlog alpha| / (sum_c |S| scale[p, c] + 2 sa[p])
omega is an INPUT of the kernels: both oracle H and the GPU get oracle R's omega rounded to float64, and each its own refits.

Tolerances are measured, not chosen: ``python tests/candidate_cvgrad_cases.py`` prints what oracle H differs from oracle R by
over the sweep (and the Ta golden rows), recorded below as MEASURED_*; every GPU bar is 10 x its constant.
"""
import functools
import os
import sys

import numpy as np

import candidate_cv_cases as cc

ROOT = cc.ROOT
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import candidates_cv_grad as cg  # noqa: E402

LD = np.longdouble
OWN = "c9"                                               # K = 31, C = 9: the unrolled-by-8 combination plus a tail; a type of weight 0
CASES = cc.SWEEP_CASES + [OWN]
OWN_K, OWN_F, OWN_C = 31, 3, 9
P = cc.SWEEP_P

# Measured by ``python tests/candidate_cvgrad_cases.py`` (oracle H against oracle R, worst over the cases named):
#   sweep: CASES x 17 candidates x 3 folds x both alphas x both metrics;  Ta: the golden rows, 8 candidates x 5 folds, both solvers
MEASURED_G = 3.0e-14
MEASURED_LAMBDA = 1.0e-11
MEASURED_GRAD = 2.4e-14
MEASURED_ALPHA = 3.3e-12
MEASURED_INVARIANT = 1.8e-16
MEASURED_G_TA = 7.2e-12
MEASURED_LAMBDA_TA = 1.1e-09
MEASURED_GRAD_TA = 3.9e-12
MEASURED_ALPHA_TA = 1.5e-10
MEASURED_INVARIANT_TA = 4.6e-17
G_BAR, LAMBDA_BAR, GRAD_BAR, ALPHA_BAR, INVARIANT_BAR = (10 * MEASURED_G, 10 * MEASURED_LAMBDA, 10 * MEASURED_GRAD,
                                                         10 * MEASURED_ALPHA, 10 * MEASURED_INVARIANT)
G_BAR_TA, LAMBDA_BAR_TA, GRAD_BAR_TA, ALPHA_BAR_TA, INVARIANT_BAR_TA = (10 * MEASURED_G_TA, 10 * MEASURED_LAMBDA_TA,
                                                                        10 * MEASURED_GRAD_TA, 10 * MEASURED_ALPHA_TA,
                                                                        10 * MEASURED_INVARIANT_TA)
TA_WEIGHTS = {"Energy": 1.0, "Force": 0.3, "Stress": 0.01}


@functools.lru_cache(maxsize=None)
def own_case():
    """(A, b, w0, composite category per row, K): K = 31 with F = 3 folds of C = 9 categories; (fold 0, category 2) and
    (fold 1, category 7) hold no row; built like ``cc.sweep_case``."""
    K = OWN_K
    sizes = np.array([[K + 13 + (f + c) % 3 for c in range(OWN_C)] for f in range(OWN_F)])
    sizes[0, 2] = sizes[1, 7] = 0
    rng = np.random.default_rng(7931)
    ccat = np.concatenate([np.full(int(n), i, dtype=np.int32) for i, n in enumerate(sizes.ravel())] + [np.full(3, -1, dtype=np.int32)])
    rng.shuffle(ccat)
    m = len(ccat)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, K)
    A = rng.standard_normal((m, K)) * scale
    truth = rng.standard_normal(K) / scale
    b = A @ truth + 0.1 * rng.standard_normal(m)
    w0 = rng.uniform(0.5, 2.0, m)
    return np.ascontiguousarray(A), b, w0, ccat, K


def case(name):
    """(A, b, w0, ccat, K, F, C, S, type of every category, weight of every type) of a case.  Sweep cases: even categories
    are energy rows (weight 1), odd ones force rows (0.3), as ``labelled`` names them; the own case: category c has type
    c % 3 with weights (1, 0.3, 0) -- the third type takes no part."""
    if name == OWN:
        A, b, w0, ccat, K = own_case()
        return A, b, w0, ccat, K, OWN_F, OWN_C, cc.ga_scales(P, OWN_C, 4242), np.arange(OWN_C) % 3, np.array([1.0, 0.3, 0.0])
    A, b, w0, ccat, K = cc.sweep_case(name)
    return A, b, w0, ccat, K, cc.SWEEP_F, cc.SWEEP_C, cc.sweep_scales(name), np.arange(cc.SWEEP_C) % 2, np.array([1.0, 0.3])


def case_alpha(name, ialpha):
    A, b, w0, ccat, K, F, C = case(name)[:7]
    return cc.base_alpha(cc.blocks_numpy(A, b, w0, ccat, F * C), K, cc.ALPHA_FRACTIONS[ialpha])


# ---- oracle R ---------------------------------------------------------------------------------------------------------
def refits_ld(bl, S, F, C, K, alpha):
    """(P, F, K) long-double refits of oracle R."""
    coef = np.zeros((S.shape[0], F, K), dtype=LD)
    for p in range(S.shape[0]):
        for f in range(F):
            coef[p, f] = cc.refit_ld(bl, S[p], f, F, C, K, alpha)
    return coef


def objective_ld(E, n, tof, wt, metric):
    """(J (P,), omega (P, C)) in long double from E (P, C): the base-weighted held-out sum (w0 r)^2 per category, n (C,) rows per
    category, tof (C,) the type of every category (-1: takes no part) and wt the weight of every type."""
    E, n = np.asarray(E, dtype=LD), np.asarray(n, dtype=LD)
    J = np.zeros(E.shape[0], dtype=LD)
    omega = np.zeros(E.shape, dtype=LD)
    for t in range(len(wt)):
        of = tof == t
        nt = n[of].sum()
        if wt[t] == 0.0 or nt == 0:
            continue
        mean = E[:, of].sum(axis=1) / nt
        if metric == "rmse":
            J += LD(wt[t]) * np.sqrt(mean)
            omega[:, of] = (LD(wt[t]) / (2 * np.sqrt(mean)) / nt)[:, None]
        else:
            J += LD(wt[t]) * mean
            omega[:, of] = LD(wt[t]) / nt
    return J, omega


def cost_ld(A, b, w0, ccat, S, F, C, alpha, tof, wt, metric):
    """J (P,) of oracle R in long double from the rows: the refits, the held-out residuals and the objective."""
    K = A.shape[1]
    bl = cc.blocks_ld(A, b, w0, ccat, F * C)
    coef = refits_ld(bl, S, F, C, K, alpha)
    E = heldout_ld(A, b, w0, ccat, coef, F, C)
    n = np.bincount(ccat[ccat >= 0], minlength=F * C).reshape(F, C).sum(axis=0)
    return objective_ld(E, n, tof, wt, metric)[0]


def heldout_ld(A, b, w0, ccat, coef, F, C):
    """(P, C) long double: sum (w0 r)^2 of the held-out rows per category, r under the long-double refit of the row's fold."""
    out = np.zeros((coef.shape[0], C), dtype=LD)
    for cci in range(F * C):
        r_ = np.flatnonzero(ccat == cci)
        if not len(r_):
            continue
        Ar, br, wr = np.asarray(A[r_], dtype=LD), np.asarray(b[r_], dtype=LD), np.asarray(w0[r_], dtype=LD)
        for p in range(coef.shape[0]):
            wres = wr * (br - Ar @ coef[p, cci // C])
            out[p, cci % C] += wres @ wres
    return out


def adjoint_ld(bl, S, omega, coef, F, C, K, alpha):
    """The adjoint formulas in long double: dict of g, sg, lam (P, F, K), grad, scale (P, C), gla, sa (P,)."""
    KK = K * K
    B = np.asarray(bl, dtype=LD).reshape(F, C, -1)
    R = B.sum(axis=0)[None] - B
    BG, Br, RG, Rr = B[:, :, :KK].reshape(F, C, K, K), B[:, :, KK:KK + K], R[:, :, :KK].reshape(F, C, K, K), R[:, :, KK:KK + K]
    Pn = S.shape[0]
    g, sg, lam = (np.zeros((Pn, F, K), dtype=LD) for _ in range(3))
    grad, scale = np.zeros((Pn, C), dtype=LD), np.zeros((Pn, C), dtype=LD)
    gla, sa = np.zeros(Pn, dtype=LD), np.zeros(Pn, dtype=LD)
    for p in range(Pn):
        for f in range(F):
            beta = coef[p, f]
            for c in range(C):
                g[p, f] += 2 * omega[p, c] * (BG[f, c] @ beta - Br[f, c])
                sg[p, f] += 2 * np.abs(omega[p, c]) * (np.abs(BG[f, c]) @ np.abs(beta) + np.abs(Br[f, c]))
            G, _ = cc.system_ld(bl, S[p], f, F, C, K)
            live = np.diag(G) > 0
            if live.any():
                H = G[np.ix_(live, live)] + LD(alpha) * np.eye(int(live.sum()), dtype=LD)
                d = np.sqrt(np.diag(H))
                lam[p, f, live] = cc.chol_solve_ld(H / d[:, None] / d[None, :], g[p, f, live] / d) / d
            la = lam[p, f]
            for c in range(C):
                grad[p, c] += la @ (Rr[f, c] - RG[f, c] @ beta)
                scale[p, c] += np.abs(la) @ (np.abs(Rr[f, c]) + np.abs(RG[f, c]) @ np.abs(beta))
            gla[p] += la @ beta
            sa[p] += np.abs(la) @ np.abs(beta)
    Sl = np.asarray(S, dtype=LD)
    return {"g": g, "sg": sg, "lam": lam, "grad": 2 * Sl * grad, "scale": 2 * np.abs(Sl) * scale, "gla": -LD(alpha) * gla,
            "sa": LD(alpha) * sa}


def oracle_from(A, b, w0, ccat, S, F, C, alpha, tof, wt, metric):
    """Oracle R of one setting: the dict of ``adjoint_ld`` plus coef (long double), omega and J."""
    K = A.shape[1]
    bl = cc.blocks_ld(A, b, w0, ccat, F * C)
    coef = refits_ld(bl, S, F, C, K, alpha)
    n = np.bincount(ccat[ccat >= 0], minlength=F * C).reshape(F, C).sum(axis=0)
    J, omega = objective_ld(heldout_ld(A, b, w0, ccat, coef, F, C), n, tof, wt, metric)
    out = adjoint_ld(bl, S, omega, coef, F, C, K, alpha)
    out.update(coef=coef, omega=omega, J=J, alpha=alpha)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, ialpha, metric="rmse"):
    """Oracle R of a case at ``cc.ALPHA_FRACTIONS[ialpha]``, computed once and shared."""
    A, b, w0, ccat, K, F, C, S, tof, wt = case(name)
    return oracle_from(A, b, w0, ccat, S, F, C, case_alpha(name, ialpha), tof, wt, metric)


# ---- the measured quantities ------------------------------------------------------------------------------------------
def f64(x):
    return np.asarray(x, dtype=np.float64)


def scaled_error(x, ref, scale):
    """max |x - ref| / scale over the entries with a scale; an entry whose scale is 0 (a category without a row there, S = 0)
    must be met exactly."""
    err, scale = np.abs(np.asarray(x) - f64(ref)), f64(scale)
    assert np.all(err[scale == 0] == 0)
    return float(np.max(err[scale > 0] / scale[scale > 0])) if np.any(scale > 0) else 0.0


def errors(ref, g, lam, grad, gla, S):
    """(g, lambda, grad_S, alpha, invariant) errors of one result against the oracle dict ``ref``; see the module docstring."""
    sa = f64(ref["sa"])
    kg = scaled_error(g, ref["g"], ref["sg"])
    lr = f64(ref["lam"])
    kl = float(np.max(np.max(np.abs(lam - lr), axis=-1) / np.maximum(np.max(np.abs(lr), axis=-1), 1e-300)))
    kd = scaled_error(grad, ref["grad"], ref["scale"])
    if np.all(sa == 0):
        assert np.all(gla == 0)
        ka = 0.0
    else:
        ka = float(np.max(np.abs(gla - f64(ref["gla"])) / sa))
    return kg, kl, kd, ka, invariant_error(ref, grad, gla, S)


def invariant_error(ref, grad, gla, S):
    """The scale invariant sum_c S dJ/dS = -2 dJ/dlog alpha, in units of the oracle's scales."""
    scale, sa = f64(ref["scale"]), f64(ref["sa"])
    return float(np.max(np.abs((S * grad).sum(axis=1) + 2 * gla) / ((np.abs(S) * scale).sum(axis=1) + 2 * sa)))


def host_result(blocks, S, omega, F, C, K, alpha):
    """Oracle H: (g, lam, grad_S, gla) of ``host_gradient`` on the refits of ``cc.host_cv``; all problems must have status 0."""
    coef, info = cc.host_cv(blocks, S, F, C, K, alpha)
    assert not info[:, :, 0].any() and info[:, :, 1].min() > cc.PIVOT_FLOOR
    grad, gla, lam, g, ginfo = cg.host_gradient(blocks, S, omega, coef, F, C, K, alpha)
    assert not ginfo[:, :, 0].any()
    return g, lam, grad, gla


# ---- the Ta golden case ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ta_oracle(name, metric="rmse"):
    """Oracle R of the golden rows for solver ``name`` (``cc.ta_oracle``'s layout and scales, base weight 1, TA_WEIGHTS)."""
    _, _, _, S, keys, ccat, bl = cc.ta_oracle(name)
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    C, K, alpha = len(keys), A.shape[1], cc.TA_ALPHAS[name]
    row_types = sorted({k[2] for k in keys})
    tof = np.array([-1 if k[1] else row_types.index(k[2]) for k in keys])
    wt = np.array([TA_WEIGHTS[t] for t in row_types])
    coef = refits_ld(bl, S, cc.TA_F, C, K, alpha)
    n = np.bincount(ccat[ccat >= 0], minlength=cc.TA_F * C).reshape(cc.TA_F, C).sum(axis=0)
    J, omega = objective_ld(heldout_ld(A, b, np.ones(len(b)), ccat, coef, cc.TA_F, C), n, tof, wt, metric)
    out = adjoint_ld(bl, S, omega, coef, cc.TA_F, C, K, alpha)
    out.update(coef=coef, omega=omega, J=J, alpha=alpha, S=S, keys=keys, ccat=ccat)
    return out


def measure():
    """Prints what the MEASURED_* constants record."""
    worst = np.zeros(5)
    for name in CASES:
        A, b, w0, ccat, K, F, C, S, tof, wt = case(name)
        blocks = cc.blocks_numpy(A, b, w0, ccat, F * C)
        for ia in range(len(cc.ALPHA_FRACTIONS)):
            for metric in cg.METRICS:
                ref = oracle(name, ia, metric)
                k = errors(ref, *host_result(blocks, S, f64(ref["omega"]), F, C, K, ref["alpha"]), S)
                print(f"{name:>6s} alpha {ref['alpha']:.2e} {metric:4s}  g {k[0]:.2e}  lambda {k[1]:.2e}  grad {k[2]:.2e}  "
                      f"alpha {k[3]:.2e}  invariant {k[4]:.2e}", flush=True)
                worst = np.maximum(worst, k)
    print("MEASURED_G = {:.1e}  MEASURED_LAMBDA = {:.1e}  MEASURED_GRAD = {:.1e}  MEASURED_ALPHA = {:.1e}  "
          "MEASURED_INVARIANT = {:.1e}".format(*worst))
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    worst = np.zeros(5)
    for name in cc.TA_ALPHAS:
        ref = ta_oracle(name)
        S, C, K = ref["S"], len(ref["keys"]), A.shape[1]
        blocks = cc.blocks_numpy(A, b, np.ones(len(b)), ref["ccat"], cc.TA_F * C)
        coef, info = cc.host_cv(blocks, S, cc.TA_F, C, K, ref["alpha"])
        assert not info[:, :, 0].any()
        grad, gla, lam, g, ginfo = cg.host_gradient(blocks, S, f64(ref["omega"]), coef, cc.TA_F, C, K, ref["alpha"])
        assert not ginfo[:, :, 0].any()
        k = errors(ref, g, lam, grad, gla, S)
        print(f"Ta {name:5s}  g {k[0]:.2e}  lambda {k[1]:.2e}  grad {k[2]:.2e}  alpha {k[3]:.2e}  invariant {k[4]:.2e}", flush=True)
        worst = np.maximum(worst, k)
    print("MEASURED_G_TA = {:.1e}  MEASURED_LAMBDA_TA = {:.1e}  MEASURED_GRAD_TA = {:.1e}  MEASURED_ALPHA_TA = {:.1e}  "
          "MEASURED_INVARIANT_TA = {:.1e}".format(*worst))


if __name__ == "__main__":
    measure()
