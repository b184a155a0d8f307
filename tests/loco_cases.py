"""Synthetic configurations shared by tests/test_gpu_loco.py and tests/loco_dist_worker.py: rows in units (configurations)
of given sizes, labels of the reference's fitsnap_dict, and brute-force leave-one-unit-out predictions by downdated
solves (G - X_c^T X_c + alpha I) beta = c - X_c^T y_c, which is the refit without the unit's rows.

For the kernel tests the same refit in long double (``Refit``, ``brute_force_ld``: an own column-oriented Cholesky, numpy has
no long-double linalg), the long-double intermediates of a unit (``unit_reference``), the a-priori rounding bar
(``kernel_bar``) and the geometry sweep of tests/test_gpu_loco.py and tests/test_loco_cpu.py (``SWEEP_K``, ``sweep_js``,
``sweep_rows``, ``sweep_units``, ``sweep_factor``, ``check_cell``)."""
import functools

import numpy as np

from fitsnap_amd.solvers import loco

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def config_rows(seed, K, sizes, testing_frac=0.0):
    rng = np.random.default_rng(seed)
    m = int(sum(sizes))
    A = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    testing = rng.random(m) < testing_frac
    labels = {
        "Configs": [f"cfg{c}" for c in cfg],
        "Groups": [f"g{c % 3}" for c in cfg],
        "Testing": testing.tolist(),
        "Row_Type": [("Energy", "Force", "Stress")[i % 3] for i in range(m)],
    }
    return A, b, w, labels


def downdated(A, b, w_eff, rows, alpha, G=None, c=None):
    """Prediction of the rows ``rows`` by the fit without them (ridge alpha; alpha = 0 is the least-squares fit)."""
    Aw, bw = A * w_eff[:, None], b * w_eff
    if G is None:
        G, c = Aw.T @ Aw, Aw.T @ bw
    Xc, yc = Aw[rows], bw[rows]
    beta = np.linalg.solve(G - Xc.T @ Xc + alpha * np.eye(A.shape[1]), c - Xc.T @ yc)
    return A[rows] @ beta


# ---- long-double reference ------------------------------------------------------------------------------------------------

def need_long_double():
    if np.finfo(LD).eps > 2e-19:
        raise RuntimeError(f"np.longdouble has eps = {np.finfo(LD).eps}: the LOCO reference needs an extended-precision "
                           "long double (eps <= 2e-19)")


def cholesky_ld(H):
    """(L, pivots, ok) of the unpivoted Cholesky H = L L^T in long double, column by column (left-looking: column j is
    H[j:, j] - L[j:, :j] L[j, :j], one vectorised product).  ``pivots``: the squared diagonal before the square root; at the
    first pivot that is not positive the factorisation stops, ok is False and that pivot fills the rest (as
    loco._cholesky_pivots)."""
    H = np.asarray(H, dtype=LD)
    d = H.shape[0]
    L = np.zeros((d, d), dtype=LD)
    piv = np.empty(d, dtype=LD)
    for j in range(d):
        col = H[j:, j] - L[j:, :j] @ L[j, :j]
        piv[j:] = col[0]
        if not col[0] > 0:
            return L, piv, False
        L[j:, j] = col / np.sqrt(col[0])
    return L, piv, True


def solve_ld(H, r):
    """x with H x = r for a symmetric positive definite H, in long double (LinAlgError when it is not)."""
    L, _, ok = cholesky_ld(H)
    if not ok:
        raise np.linalg.LinAlgError("cholesky_ld: not positive definite")
    x = np.array(r, dtype=LD)
    d = x.shape[0]
    for k in range(d):
        x[k] /= L[k, k]
        x[k + 1:] -= L[k + 1:, k] * x[k]
    for k in range(d - 1, -1, -1):
        x[k] /= L[k, k]
        x[:k] -= L[k, :k] * x[k]
    return x


class Refit:
    """Long-double refits without a unit, sharing the statistics of all rows over the units: G = X^T X, c = X^T y
    (X = w a, y = w b) once, then per unit G_-c = G - X_c^T X_c, c_-c = c - X_c^T y_c and a full solve -- a refit, not the
    Woodbury algebra.  With a factor M (K x J, J < K; or ``projected``) the refit runs in the projected features
    zeta = a M: M^T (G_-c + alpha I) M gamma = M^T c_-c, prediction A_c M gamma (the fit being beta = M M^T c).
    ``project_rows``: the projected statistics from the projected rows X M themselves instead of M^T G M -- for an M with
    huge columns (an ill-conditioned fit), where the products with G would lose what long double has."""

    def __init__(self, A, b, w_eff, alpha, M=None, stats=None, projected=None, project_rows=False):
        need_long_double()
        self.A = np.asarray(A)
        self.w = np.asarray(w_eff).astype(LD)
        self.y = self.w * np.asarray(b).astype(LD)
        K = self.A.shape[1]
        alpha = LD(alpha)
        self.M = None
        if projected is None:
            projected = M is not None and np.shape(M)[1] < K
        if projected:
            self.M = np.asarray(M).astype(LD).reshape(K, -1)
            if project_rows:
                T = (self.A.astype(LD) * self.w[:, None]) @ self.M
                self.P = T.T @ T + alpha * (self.M.T @ self.M)
                self.q = T.T @ self.y
            else:
                G, c = stats if stats is not None else stats_ld(A, b, w_eff)
                self.P = self.M.T @ ((G + alpha * np.eye(K, dtype=LD)) @ self.M)
                self.q = self.M.T @ c
        else:
            G, self.c = stats if stats is not None else stats_ld(A, b, w_eff)
            self.Ga = G + alpha * np.eye(K, dtype=LD)

    def predict(self, rows, zeta=None):
        """Predictions of the rows ``rows`` by the fit without them (float64); ``zeta``: A[rows] M in long double when
        the caller has it already."""
        Ac = self.A[rows].astype(LD)
        w, yc = self.w[rows, None], self.y[rows]
        if self.M is None:
            Xc = Ac * w
            return (Ac @ solve_ld(self.Ga - Xc.T @ Xc, self.c - Xc.T @ yc)).astype(np.float64)
        if zeta is None:
            zeta = Ac @ self.M
        T = zeta * w
        return (zeta @ solve_ld(self.P - T.T @ T, self.q - T.T @ yc)).astype(np.float64)


def stats_ld(A, b, w_eff):
    """(G, c) of the weighted rows in long double."""
    w = np.asarray(w_eff).astype(LD)
    X = np.asarray(A).astype(LD) * w[:, None]
    return X.T @ X, X.T @ (w * np.asarray(b).astype(LD))


def brute_force_ld(A, b, w_eff, rows_of_unit, alpha, M=None):
    """Prediction of the rows ``rows_of_unit`` by the fit without them, in long double (see ``Refit``; float64 out)."""
    return Refit(A, b, w_eff, alpha, M).predict(np.asarray(rows_of_unit))


def unit_reference(A, b, w_eff, rows, M, beta, precise=True):
    """The intermediates of one unit with the M and beta the kernel gets, in long double (``precise``; float64 otherwise,
    enough for a bar): dict with "d" = min(n, J), "nspace", "piv" (smallest Cholesky pivot of H_c = I - Z_c Z_c^T (n <= J) or
    I - Z_c^T Z_c, up to and including the first one at or below loco.PIVOT_TOL, where the kernel stops; NaN without
    ``precise``), "lam_min"
    (1 - lambda_max(S_c)), "zeta" (A_c M), "v" (v_c, None when H_c is not positive definite) and "bar" (``kernel_bar`` of
    the unit's rows, None likewise)."""
    T = LD if precise else np.float64
    if precise:
        need_long_double()
    M = np.asarray(M, dtype=np.float64).reshape(np.shape(A)[1], -1)
    K, J = M.shape
    Ac = np.asarray(A)[rows]
    n = len(rows)
    w = np.asarray(w_eff)[rows].astype(T)
    zeta = Ac.astype(T) @ M.astype(T)
    Z = w[:, None] * zeta
    e = w * np.asarray(b)[rows].astype(T) - w * (Ac.astype(T) @ np.asarray(beta).astype(T))
    nspace = n <= J
    d = min(n, J)
    S = Z @ Z.T if nspace else Z.T @ Z
    H = np.eye(d, dtype=T) - S
    out = {"d": d, "nspace": nspace, "zeta": zeta, "v": None, "bar": None,
           "lam_min": 1.0 - float(np.linalg.eigvalsh(S.astype(np.float64))[-1])}
    if precise:
        _, piv, ok = cholesky_ld(H)
        low = np.flatnonzero(~(piv > loco.PIVOT_TOL))
        out["piv"] = float(piv[:low[0] + 1].min() if low.size else piv.min())
    else:
        out["piv"] = np.nan
        try:
            np.linalg.cholesky(H)
            ok = True
        except np.linalg.LinAlgError:
            ok = False
    if ok and out["lam_min"] > 0.0:
        rhs = e if nspace else Z.T @ e
        u = solve_ld(H, rhs) if precise else np.linalg.solve(H, rhs)
        out["v"] = (Z.T @ u if nspace else u).astype(np.float64)
        out["bar"] = kernel_bar(Ac, M, beta, out["v"], out["lam_min"], d)
    return out


def kernel_bar(Ac, M, beta, v, lam_min, d):
    """A-priori rounding bar of the LOO predictions p_i = a_i . beta - zeta_i . v_c of one unit's rows ``Ac``, per row:

        4 eps [ K (|a_i| . |beta|) + (K + J + d_c) ((|a_i| |M|) . |v_c|) / lambda_min(H_c) ]

    built from the inputs and the REFERENCE's intermediates only (v_c and lambda_min(H_c) = 1 - lambda_max(S_c) come from
    ``unit_reference``, never from the kernel).  Derivation, with gamma_k ~ k eps the bound of a serial FMA chain of length k:
    a_i . beta is a chain of length K (4 interleaved chains of K / 4 and a two-step tree on the device: shorter), error
    <= gamma_K |a_i| . |beta|.  zeta_i = a_i M is a chain of length K per entry (the MFMA accumulates the k index in order),
    error <= gamma_K |a_i| |M|; zeta_i . v is a chain of length J, so with an exact v the second product errs by
    <= gamma_{K + J} (|a_i| |M|) . |v|.  v itself solves H_c u = rhs by a Cholesky of order d_c: backward stable, relative
    error <= gamma_{d_c} kappa(H_c), and kappa(H_c) = lambda_max / lambda_min <= 1 / lambda_min(H_c) since H_c = I - S_c with
    S_c positive semi-definite has lambda_max(H_c) <= 1; the errors of H_c's and the right-hand side's own entries (chains of
    length J or n_c over products of zeta) enter v through the same 1 / lambda_min.  Together
    (K + J + d_c) eps (|a_i| |M|) . |v_c| / lambda_min; the constant 4 is that of select_cases.kernel_bar (two roundings per
    FMA chain step counted separately, and a factor 2 of slack).

    Measured on an MI355X by tests/test_gpu_loco.py's sweep (every cell prints its line).  Per (K, J), worst over
    alpha = 0, 1e-8, 1e-4: worst row error / bar, then the kernel's RMS error over loco_host's RMS error, both against the
    long-double refit (J = K: factor_cholesky; J < K: factor_eigen(rank=J)):

    K =   1  J=1: 0.45 / 1
    K =   2  J=2: 0.21 / 1.1
    K =  15  J=15: 0.017 / 1
    K =  16  J=16: 0.019 / 1
    K =  17  J=17: 0.018 / 0.99  J=1: 0.15 / 1.1  J=15: 0.12 / 1  J=9: 0.08 / 1  J=16: 0.11 / 1
    K =  31  J=31: 0.0098 / 1  J=1: 0.044 / 1  J=15: 0.046 / 1  J=17: 0.046 / 1  J=30: 0.076 / 1
    K =  32  J=32: 0.0087 / 1  J=1: 0.033 / 1  J=15: 0.057 / 1  J=17: 0.047 / 1  J=31: 0.064 / 1
    K =  33  J=33: 0.0064 / 1  J=1: 0.062 / 2.1  J=15: 0.045 / 1  J=17: 0.044 / 1  J=32: 0.084 / 1
    K =  64  J=64: 0.0037 / 1  J=1: 0.017 / 1.1  J=15: 0.016 / 1  J=17: 0.017 / 1  J=33: 0.015 / 1  J=63: 0.021 / 1
    K = 110  J=110: 0.0019 / 1  J=1: 0.014 / 1  J=15: 0.0062 / 1  J=17: 0.0063 / 1  J=55: 0.007 / 1  J=109: 0.011 / 1
    K = 128  J=128: 0.0014 / 1  J=1: 0.005 / 1  J=15: 0.005 / 1  J=17: 0.0067 / 1  J=65: 0.0076 / 1  J=127: 0.01 / 1
    K = 142  J=142: 0.0012 / 1  J=1: 0.0095 / 1.3  J=15: 0.0058 / 1  J=17: 0.0054 / 1  J=71: 0.0044 / 1  J=141: 0.01 / 1
    K = 144  J=144: 0.0013 / 1  J=1: 0.0037 / 0.99  J=15: 0.0033 / 1  J=17: 0.0035 / 1  J=73: 0.0051 / 1  J=143: 0.009 / 1
    K = 145  J=145: 0.0014 / 0.99  J=1: 0.0051 / 1.1  J=15: 0.005 / 1  J=17: 0.0051 / 1  J=73: 0.0045 / 1  J=144: 0.009 / 1
    K = 150  J=150: 0.0018 / 0.97  J=1: 0.011 / 1.1  J=15: 0.0048 / 1  J=17: 0.0043 / 1  J=75: 0.0041 / 1  J=149: 0.0099 / 1
    K = 231  J=231: 0.001 / 1  J=1: 0.0015 / 1.9  J=15: 0.0027 / 1  J=17: 0.0021 / 1  J=115: 0.0025 / 1  J=230: 0.0038 / 1
    K = 256  J=256: 0.0008 / 1  J=1: 0.0021 / 1.1  J=15: 0.002 / 1  J=17: 0.0018 / 1  J=129: 0.0029 / 1  J=255: 0.0049 / 1
    K = 290  J=290: 0.00083 / 1  J=1: 0.0024 / 1.2  J=15: 0.0016 / 1  J=17: 0.0014 / 1  J=145: 0.0021 / 1  J=289: 0.0039 / 1
    K = 480  J=480: 0.00051 / 1  J=1: 0.00075 / 1.1  J=15: 0.00092 / 1  J=17: 0.00091 / 1  J=241: 0.00096 / 1  J=479: 0.0018 / 1

    Worst error / bar 0.45 (K = 1, where the bar is 12 eps wide); worst RMS ratio 2.12 (K = 33, J = 1, where both errors
    are 1e-16: a few last-bit differences of a . beta).  Layout cases: 0.03 / 1.0; 20 000 units: 0.012 / 1.02; every unit of
    the 10^6-row case against loco_host: 0.0022.  RMS_FACTOR below is 2 x 2.12 rounded up to a power of two.
    """
    aa = np.abs(np.asarray(Ac, dtype=np.float64))
    M = np.abs(np.asarray(M, dtype=np.float64)).reshape(aa.shape[1], -1)
    K, J = M.shape
    return 4 * EPS * (K * (aa @ np.abs(np.asarray(beta, dtype=np.float64)))
                      + (K + J + d) * ((aa @ M) @ np.abs(np.asarray(v, dtype=np.float64))) / lam_min)


# ---- the geometry sweep ---------------------------------------------------------------------------------------------------

SWEEP_K = [1, 2, 15, 16, 17, 31, 32, 33, 64, 110, 128, 142, 144, 145, 150, 231, 256, 290, 480]
SWEEP_ALPHA = [0.0, 1e-8, 1e-4]
BOUNDARY = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 420]   # plus J - 1, J, J + 1 per cell
FILL = 150                   # size of the filler units that bring m to >= 5 K
LAM_MIN = 0.05               # every unit of the sweep has lambda_min(H_c) >= this in the reference
LD_ALL_BELOW = 256           # K >= this: long-double refits for the boundary-size units only, loco_host for the fillers
RMS_FACTOR = 8.0             # kernel RMS error <= this x loco_host's (both against long double), per cell: 2 x the worst
                             # measured ratio (2.12, see kernel_bar) rounded up to a power of two; may never exceed 16


def sweep_js(K):
    """J = K (factor_cholesky) and, for K >= 17, J < K from factor_eigen(rank=J)."""
    js = [K]
    if K >= 17:
        js += [J for J in dict.fromkeys((1, 15, 17, (K // 2) | 1, K - 1)) if J < K]
    return js


@functools.lru_cache(maxsize=None)
def sweep_rows(K):
    """(A, b, w, G, c, (G, c) in long double) of the sweep's rows at K: config_rows-style, m >= 5 K and enough for every
    boundary size, J - 1, J, J + 1 and one filler."""
    m = max(5 * K, sum(BOUNDARY) + 3 * K + FILL)
    A, b, w, _ = config_rows(1000 + K, K, [m])
    Aw = A * w[:, None]
    return A, b, w, Aw.T @ Aw, Aw.T @ (b * w), stats_ld(A, b, w)


def sweep_units(K, J, m):
    """(offsets int64, boundary mask per unit) of the cell's units over the rows 0 ... m - 1 in row order: the boundary sizes
    and J - 1, J, J + 1, fillers of FILL rows (the last one takes the rest), in shuffled order."""
    sizes = BOUNDARY + [n for n in (J - 1, J, J + 1) if n >= 1]
    rest = m - sum(sizes)
    assert rest >= 0
    fill = [FILL] * (rest // FILL)
    if rest % FILL:
        fill.append(rest % FILL)
    allsizes = np.array(sizes + fill)
    boundary = np.arange(len(allsizes)) < len(sizes)
    order = np.random.default_rng(7 * K + J).permutation(len(allsizes))
    return np.concatenate([[0], np.cumsum(allsizes[order])]).astype(np.int64), boundary[order]


def sweep_factor(G, c, alpha, J, stats):
    """(M, beta) of a cell: J = K from factor_cholesky with beta = (G + alpha I)^-1 c; J < K from factor_eigen(rank=J) with
    beta = M M^T c.  beta is computed in long double on the long-double statistics (``stats``) and rounded once: the bar
    bounds the kernel's own rounding of a . beta by 4 K eps, and a float64 beta is itself off by more than that where K is
    tiny (5 eps at K = 2) or where M^T c cancels (by a factor of several hundred at J = 1)."""
    K = G.shape[0]
    if J == K:
        beta = solve_ld(stats[0] + LD(alpha) * np.eye(K, dtype=LD), stats[1])
        return loco.factor_cholesky(G, alpha), beta.astype(np.float64)
    M = loco.factor_eigen(G, alpha, rank=J)
    assert M.shape == (K, J)
    Ml = M.astype(LD)
    return M, (Ml @ (Ml.T @ stats[1])).astype(np.float64)


def measure_cell(A, b, w_eff, alpha, M, beta, rows, off, pred, stats=None, ld_units=None, host=None, ld_bars=True,
                 **refit_options):
    """Errors of the predictions ``pred`` of one cell.  Units with ld_units[u] (default: all) are compared with the
    long-double refit, the others with loco_host (``host``), every row against the a-priori bar of its unit (from
    long-double intermediates; from float64 ones for the loco_host units with ld_bars = False, whose "piv" is NaN then).
    dict of per-unit arrays "ratio" (worst row error / bar; inf where the reference H_c is not positive definite or a
    prediction is not finite), "lam_min", "piv", "d", "nspace", "abs" (worst row error), the per-row arrays "truth" (what the
    row was compared with) and "bar", and the scalars "rms_pred", "rms_host" (RMS error of ``pred`` and of loco_host over
    the long-double rows)."""
    ncfg = len(off) - 1
    if host is None:
        host = loco.loco_host(A, b, w_eff, M, beta, rows, off)[0]
    refit = None                                    # built at the first long-double unit: its statistics cost m K^2
    out = {k: np.zeros(ncfg) for k in ("ratio", "lam_min", "piv", "d", "nspace", "abs")}
    out["truth"] = np.full(np.shape(A)[0], np.nan)
    out["bar"] = np.full(np.shape(A)[0], np.nan)
    se_pred = se_host = 0.0
    nld = 0
    for u in range(ncfg):
        r = np.asarray(rows[off[u]:off[u + 1]])
        ld = ld_units is None or bool(ld_units[u])
        ref = unit_reference(A, b, w_eff, r, M, beta, precise=ld or ld_bars)
        for k in ("lam_min", "d", "nspace"):
            out[k][u] = ref[k]
        out["piv"][u] = ref["piv"]
        if ref["bar"] is None:
            out["ratio"][u] = out["abs"][u] = np.inf
            continue
        if ld:
            if refit is None:
                refit = Refit(A, b, w_eff, alpha, M, stats, **refit_options)
            truth = refit.predict(r, ref["zeta"] if refit.M is not None else None)
            se_pred += float(np.sum((pred[r] - truth) ** 2))
            se_host += float(np.sum((host[r] - truth) ** 2))
            nld += len(r)
        else:
            truth = host[r]
        out["truth"][r] = truth
        out["bar"][r] = ref["bar"]
        err = np.abs(pred[r] - truth)
        err[~np.isfinite(err)] = np.inf
        out["ratio"][u] = np.max(err / ref["bar"])
        out["abs"][u] = np.max(err)
    out["rms_pred"] = np.sqrt(se_pred / max(nld, 1))
    out["rms_host"] = np.sqrt(se_host / max(nld, 1))
    return out


def cell_line(tag, res):
    """One line of the measured table."""
    rr = res["rms_pred"] / res["rms_host"] if res["rms_host"] > 0 else np.inf
    return (f"LOCO {tag}: worst err/bar {np.max(res['ratio']):.3g}  rms/host {rr:.3g}  "
            f"(rms {res['rms_pred']:.3g}, host {res['rms_host']:.3g})  lam_min {np.min(res['lam_min']):.3g}")
