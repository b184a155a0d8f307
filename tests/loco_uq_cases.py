"""Helpers of tests/test_loco_uq_cpu.py and tests/test_gpu_loco_uq.py: the long-double reference of the leave-one-unit-out
leverages q_i, joint distances D_c and log-determinants l_c by explicit refits without the unit (``RefitUQ``, on
loco_cases.Refit / cholesky_ld / stats_ld), the a-priori rounding bars (``uq_bars``) and the per-cell measurement
(``measure_cell``, ``cell_line``)."""
import numpy as np

import loco_cases as lc
from fitsnap_amd.solvers import loco_uq

LD = lc.LD
EPS = lc.EPS
RMS_FACTOR = 8.0             # kernel RMS error <= this x loco_uq_host's (both against long double), per cell and quantity: 2 x the
                             # worst measured ratio (3.14, see uq_bars) rounded up to a power of two; may never exceed 16


def forward_ld(L, R):
    """L^-1 R for a lower-triangular L and a matrix R, in long double (column-oriented substitution)."""
    Y = np.array(R, dtype=LD)
    for k in range(L.shape[0]):
        Y[k] /= L[k, k]
        Y[k + 1:] -= np.outer(L[k + 1:, k], Y[k])
    return Y


def logdet_ld(L):
    return 2 * np.sum(np.log(np.diag(L)))


class RefitUQ:
    """Leave-one-unit-out predictive quantities by REFITS in long double, not by the Woodbury algebra: with B_-c = G -
    X_c^T X_c + alpha I (loco_cases.Refit's downdated statistics; in the projected features zeta = a M when the fit is a
    truncated one, J < K: P - T_c^T T_c with P = M^T (G + alpha I) M)

        q_i = a_i B_-c^-1 a_i^T                          (zeta_i (P - T^T T)^-1 zeta_i^T)
        l_c = log det B_-c - log det (G + alpha I)       (= log det H_c, the matrix determinant lemma)
        D_c = sum_i [w_i (b_i - a_i . beta)] [w_i (b_i - p_i)]       beta the full fit, p_i the refit's prediction: the weighted
              leave-out residual IS H_c^-1 e_c, so this is e_c^T H_c^-1 e_c without ever forming H_c

    all from one Cholesky of B_-c per unit."""

    def __init__(self, A, b, w_eff, alpha, M=None, stats=None):
        self.refit = lc.Refit(A, b, w_eff, alpha, M, stats)
        r = self.refit
        self.base = r.P if r.M is not None else r.Ga
        self.rhs = r.q if r.M is not None else r.c
        L, _, ok = lc.cholesky_ld(self.base)
        assert ok
        self.base_logdet = logdet_ld(L)
        self.full = lc.solve_ld(self.base, self.rhs)          # the fit on all rows (in the projected features when J < K)

    def unit(self, rows):
        """dict of "pred", "q" (per row, float64) and "dist", "logdet" (float64) of the unit with the rows ``rows``."""
        r = self.refit
        F = r.A[rows].astype(LD)
        if r.M is not None:
            F = F @ r.M
        w, y = r.w[rows], r.y[rows]
        T = F * w[:, None]
        B = self.base - T.T @ T
        L, _, ok = lc.cholesky_ld(B)
        if not ok:
            raise np.linalg.LinAlgError("RefitUQ: the statistics without the unit are not positive definite")
        Y = forward_ld(L, F.T)
        g = forward_ld(L, (self.rhs - T.T @ y)[:, None])[:, 0]
        pred = Y.T @ g                                         # F B^-1 (c - T^T y)
        e = y - w * (F @ self.full)
        return {"pred": pred.astype(np.float64), "q": np.sum(Y * Y, axis=0).astype(np.float64),
                "dist": float(e @ (y - w * pred)), "logdet": float(logdet_ld(L) - self.base_logdet)}


def uq_bars(Ac, bc, wc, M, beta, lam_min, d, loo_res, logdet):
    """A-priori rounding bars (q per row, D_c, l_c) of one unit, built from the inputs and the REFERENCE's intermediates only
    (``lam_min`` = lambda_min(H_c) = 1 - lambda_max(S_c) from loco_cases.unit_reference, ``loo_res`` = the reference's weighted
    leave-out residuals H_c^-1 e_c, ``logdet`` its l_c), never from the kernel.  With s_i = |a_i| |M| (so |zeta_i| <= s_i
    entrywise), chain = K + J + d_c and the constant 4 of loco_cases.kernel_bar:

        q_i:  4 eps chain |s_i|^2 / lam_min^2
        D_c:  4 eps [ 2 (K + 2) sum_i |loo_res_i| w_i (|a_i| . |beta| + |b_i|)  +  chain |e_c|^2 / lam_min^2 ]
        l_c:  4 eps [ chain (sum_i w_i^2 |s_i|^2 + d_c) / lam_min  +  d_c |l_c| ]

    Derivation (gamma_k ~ k eps, the bound of a serial FMA chain of length k).  zeta_i = a_i M errs by gamma_K s_i per entry.
    The entries of S_c are chains of length J (n space) or over the unit's rows in MFMA steps of 4 (J space) of products of
    zeta, the Cholesky of H_c = I - S_c of order d_c is backward stable with |dH| <= gamma_{d_c} |L| |L^T|, and the
    triangular solves (or the explicit inverse of L) add gamma_{d_c} more: together a relative perturbation of H_c^-1 of at
    most chain eps kappa(H_c), and kappa(H_c) <= 1 / lam_min because lambda_max(H_c) <= 1 (loco_cases.kernel_bar).
    q_i = zeta_i H_c^-1 zeta_i^T (both forms are this number; neither subtracts): the quadratic form itself is at most
    |zeta_i|^2 / lam_min <= |s_i|^2 / lam_min -- 1 / lam_min once for the form -- and its relative error chain eps / lam_min --
    once more for the factor; the direct error of zeta, 2 gamma_K |s_i|^2 / lam_min, and the final sum of d_c squares are
    below that since lam_min <= 1.  D_c = e^T H_c^-1 e: e_i = w_i b_i - w_i (a_i . beta) errs by gamma_{K + 2} w_i (|a_i| .
    |beta| + |b_i|) (that also covers beta being the long-double fit rounded once), and dD = 2 (H^-1 e) . de to first order,
    with H^-1 e the reference's weighted leave-out residual; the perturbation of H_c^-1 gives chain eps |e|^2 / lam_min^2 as
    for q.  l_c = log det H_c: d l = tr(H_c^-1 dH) <= |dH|_* / lam_min, where the entry errors of S_c sum to at most chain
    eps sum_i w_i^2 |s_i|^2 on the trace norm (>= tr S_c) and the Cholesky's backward error to gamma_{d_c} tr(|L| |L^T|) =
    gamma_{d_c} tr H_c <= gamma_{d_c} d_c; the d_c logarithms (every L_kk <= 1: all of one sign) and their sum add
    gamma_{d_c} |l_c|.

    Measured on an MI355X by tests/test_gpu_loco_uq.py's sweep (every cell prints its line).  Per (K, J), worst over alpha = 0
    and 1e-4: worst error / bar of q, D, l, then the kernel's RMS error over loco_uq_host's for q, D, l, both against the
    long-double refit (J = K: factor_cholesky; J < K: factor_eigen(rank=J)):

    K =   1  J=1: 0.23 0.03 0.069 / 1.3 1.2 1.5
    K =   2  J=2: 0.19 0.015 0.028 / 1.2 0.69 1.2
    K =  17  J=17: 0.011 0.0032 0.0027 / 0.91 0.97 1.9  J=1: 0.11 0.0061 0.0083 / 0.9 0.9 0.76  J=15: 0.0056 0.023 0.0029 / 1 1.1 1.3  J=16: 0.006 0.025 0.0026 / 1 1 1.7
    K =  33  J=33: 0.0055 0.0012 0.0019 / 0.78 0.81 1.6  J=1: 0.022 0.0037 0.0049 / 1.4 1.3 1.1  J=15: 0.0027 0.016 0.002 / 0.98 1.1 0.89  J=32: 0.0013 0.024 0.0012 / 0.99 0.95 1.7
    K =  64  J=64: 0.0023 0.00031 0.0005 / 0.7 0.87 2.6  J=1: 0.008 0.0016 0.0022 / 1.2 1.7 0.97  J=15: 0.0014 0.003 0.0016 / 0.98 0.56 1.7  J=63: 0.00032 0.0072 0.00062 / 0.94 1 1.6
    K = 128  J=128: 0.00076 0.00046 0.00054 / 0.76 0.98 3.1  J=1: 0.0044 0.00068 0.0011 / 1.1 1.1 1  J=15: 0.0004 0.0013 0.00055 / 0.98 0.8 1.6  J=127: 8e-05 0.0037 0.00011 / 0.9 1 1.3
    K = 145  J=145: 0.00071 0.00028 0.00035 / 0.81 1.2 1.8  J=1: 0.0033 0.00077 0.001 / 2.2 2 1.3  J=15: 0.00042 0.0026 0.0004 / 0.96 0.69 1.1  J=144: 7.1e-05 0.0018 5.7e-05 / 0.93 1 2.3

    Worst error / bar 0.23 (q at K = 1, where the bar is 12 eps wide); worst RMS ratio 3.14 (l at K = J = 128, both errors
    1e-15: the kernel adds the 128 logarithms in a binary tree, numpy pairwise in blocks of 8).  A first form of the kernel
    that added the 256 per-thread partials of D_c and l_c in one chain measured 13.6 (D at J = 1) and 8.4 (l at K = 128); the
    tree brought them to 1.1 and 3.1.  RMS_FACTOR is 2 x 3.14 rounded up to a power of two.
    """
    aa = np.abs(np.asarray(Ac, dtype=np.float64))
    Ma = np.abs(np.asarray(M, dtype=np.float64)).reshape(aa.shape[1], -1)
    K, J = Ma.shape
    wc = np.asarray(wc, dtype=np.float64)
    chain = K + J + d
    s2 = np.sum((aa @ Ma) ** 2, axis=1)
    ab = aa @ np.abs(np.asarray(beta, dtype=np.float64))
    e = wc * np.asarray(bc, dtype=np.float64) - wc * (np.asarray(Ac, dtype=np.float64) @ np.asarray(beta, dtype=np.float64))
    bar_q = 4 * EPS * chain * s2 / lam_min ** 2
    bar_d = 4 * EPS * (2 * (K + 2) * np.sum(np.abs(loo_res) * wc * (ab + np.abs(bc))) + chain * (e @ e) / lam_min ** 2)
    bar_l = 4 * EPS * (chain * (np.sum(wc * wc * s2) + d) / lam_min + d * abs(logdet))
    return bar_q, bar_d, bar_l


def measure_cell(A, b, w_eff, alpha, M, beta, rows, off, lev, info, stats=None, ld_units=None, host=None):
    """Errors of the leverages ``lev`` and the per-unit (l_c, D_c) of ``info`` (columns 4, 5) of one cell.  Units with
    ld_units[u] (default: all) are compared with the long-double refit (``RefitUQ``), the others with ``loco_uq_host``
    (``host`` = its (pred, lev, info)); every number against its bar (``uq_bars``).  dict of per-unit arrays "ratio_q", "ratio_d", "ratio_l" (worst error / bar; inf
    where a number is not finite), "lam_min", the per-row "truth_pred" (NaN on the loco_uq_host units) and the scalars
    "rms_q", "rms_d", "rms_l" and "host_rms_q", ... over the long-double units."""
    ncfg = len(off) - 1
    if host is None:
        host = loco_uq.loco_uq_host(A, b, w_eff, M, beta, rows, off)
    ref = None
    out = {k: np.zeros(ncfg) for k in ("ratio_q", "ratio_d", "ratio_l", "lam_min")}
    out["truth_pred"] = np.full(np.shape(A)[0], np.nan)
    se = {k: 0.0 for k in ("q", "d", "l", "hq", "hd", "hl")}
    nrows = nunits = 0
    for u in range(ncfg):
        r = np.asarray(rows[off[u]:off[u + 1]])
        ld = ld_units is None or bool(ld_units[u])
        mid = lc.unit_reference(A, b, w_eff, r, M, beta, precise=False)     # lam_min and d only
        out["lam_min"][u] = mid["lam_min"]
        if ld:
            if ref is None:
                ref = RefitUQ(A, b, w_eff, alpha, M, stats)
            t = ref.unit(r)
            out["truth_pred"][r] = t["pred"]
            tq, td, tl = t["q"], t["dist"], t["logdet"]
            loo = w_eff[r] * (b[r] - t["pred"])
        else:
            tq, td, tl = host[1][r], host[2][u, 5], host[2][u, 4]
            loo = w_eff[r] * (b[r] - host[0][r])
        bq, bd, bl = uq_bars(A[r], b[r], w_eff[r], M, beta, mid["lam_min"], mid["d"], loo, tl)
        err = [np.abs(lev[r] - tq), abs(info[u, 5] - td), abs(info[u, 4] - tl)]
        for name, e_, bar in zip(("ratio_q", "ratio_d", "ratio_l"), err, (bq, bd, bl)):
            e_ = np.where(np.isfinite(e_), e_, np.inf)
            out[name][u] = np.max(e_ / bar)
        if ld:
            se["q"] += float(np.sum(err[0] ** 2))
            se["d"] += float(err[1] ** 2)
            se["l"] += float(err[2] ** 2)
            se["hq"] += float(np.sum((host[1][r] - tq) ** 2))
            se["hd"] += float((host[2][u, 5] - td) ** 2)
            se["hl"] += float((host[2][u, 4] - tl) ** 2)
            nrows += len(r)
            nunits += 1
    for k, n in (("q", nrows), ("d", nunits), ("l", nunits)):
        out["rms_" + k] = np.sqrt(se[k] / max(n, 1))
        out["host_rms_" + k] = np.sqrt(se["h" + k] / max(n, 1))
    return out


def cell_line(tag, res):
    """One line of the measured table."""
    def rr(k):
        return res["rms_" + k] / res["host_rms_" + k] if res["host_rms_" + k] > 0 else np.inf
    return (f"LOCO-UQ {tag}: worst err/bar q {np.max(res['ratio_q']):.3g} D {np.max(res['ratio_d']):.3g} "
            f"l {np.max(res['ratio_l']):.3g}  rms/host q {rr('q'):.3g} D {rr('d'):.3g} l {rr('l'):.3g}  "
            f"lam_min {np.min(res['lam_min']):.3g}")


def check_cell(tag, res):
    """The acceptance of one cell: (a) every number within its bar, (b) the RMS errors at most RMS_FACTOR x loco_uq_host's; the
    sweep's own promise lambda_min(H_c) >= loco_cases.LAM_MIN is asserted on the reference side."""
    print(cell_line(tag, res), flush=True)
    assert np.min(res["lam_min"]) >= lc.LAM_MIN, (tag, np.min(res["lam_min"]))
    for k in ("q", "d", "l"):
        worst = int(np.argmax(res["ratio_" + k]))
        assert res["ratio_" + k][worst] <= 1.0, (tag, k, "unit", worst, res["ratio_" + k][worst])
        assert res["rms_" + k] <= RMS_FACTOR * res["host_rms_" + k], (tag, k, res["rms_" + k], res["host_rms_" + k])
