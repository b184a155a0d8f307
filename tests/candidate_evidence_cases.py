"""Cases, oracles and tolerances of the marginal likelihood of group-weight candidates (tests/test_candidate_evidence_cpu.py,
tests/test_gpu_candidate_evidence.py).

Oracle R: long double throughout.  The per-category blocks are accumulated from the rows (``cc.blocks_ld``), the system of a
candidate is Jacobi-scaled, factored, inverted and solved by hand-written long-double loops, the residual sums Q_c come from the
ROWS (sum (w0 (b - a . beta))^2: no cancellation), and L with all its derivatives follows the definitions of
solvers/candidates_evidence.py.

Oracle D, independent of every formula there: for cases with <= 48 active rows and alpha > 0, L(fixed) is the log density of the
observed targets under N(0, diag(w_r^-2) + A A' / alpha), by a long-double Cholesky of the N x N covariance.

Error measures (every scale is taken from oracle R):
  L        |L - L_R| / N
  beta     |beta - beta_R|_2 / |beta_R|_2
  Q        |Q - Q_R| / (bb + 2 |beta| . |r| + |beta|' |G| |beta|)                (the cancellation-safe scale)
  gamma    |gamma - gamma_R| / (|S^-1|_F |G_c|_F lambda_c)
  gradient |g - g_R| / (sum of the magnitudes of its three terms), dL/dlog S and dL/dlog alpha alike
  invariants  sum_c gamma_c + alpha tr(S^-1) = k  (tr(S^-1) read back from dL/dlog alpha), and
              sum_c dL/dlog S + 2 dL/dlog alpha = 0 (profiled) or N' - R (fixed), each over the sum of the magnitudes that enter

Tolerances are measured, not chosen: ``python tests/candidate_evidence_cases.py`` prints what ``host_evidence`` (on
``cc.blocks_numpy`` blocks) differs from oracle R by over the cases (and the Ta golden rows), recorded below as MEASURED_*; every
GPU bar is 10 x its constant.
"""
import functools
import os
import sys

import numpy as np

import candidate_cv_cases as cc
import candidate_cvgrad_cases as gc

ROOT = cc.ROOT
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import candidates_evidence as ce  # noqa: E402

LD = np.longdouble
P = cc.SWEEP_P                                           # 17: three candidate tiles of 8, the last with one candidate
BATCHES = (1, 8, 9, 17)
C9, C17, ZERO = "c9", "c17", "zerocol"
OWN = [C9, C17, ZERO]
CASES = cc.SWEEP_CASES + OWN
SCALES = ce.SCALES
LOG_2PI = np.log(2 * LD(np.pi))

# Measured by ``python tests/candidate_evidence_cases.py`` (``host_evidence`` against oracle R, worst over the cases named):
#   sweep: CASES x 17 candidates x both alphas x both scales;  Ta: the golden rows, 9 candidates, both solvers' alphas, both scales
# L has one constant per scale.  Under "fixed" L holds -R / 2 with R = sum_c lambda_c Q_c, and the GA-style scales (1e-4 ... 1e7)
# say nothing about the noise: R / N reaches 1e15 (Ta: 1e21), so eps R / N is what an absolute error per row can be.  Under
# "profiled" R enters through log(R / N') and the same measure is tight.
MEASURED_L = 2.1e-10
MEASURED_L_FIXED = 1.3e-01
MEASURED_BETA = 8.7e-14
MEASURED_Q = 1.1e-15
MEASURED_GAMMA = 5.3e-16
MEASURED_GRAD = 9.2e-10
MEASURED_INVARIANT = 2.2e-10
MEASURED_L_TA = 1.2e-10
MEASURED_L_FIXED_TA = 2.0e+05
MEASURED_BETA_TA = 3.0e-11
MEASURED_Q_TA = 3.3e-13
MEASURED_GAMMA_TA = 8.8e-20
MEASURED_GRAD_TA = 6.6e-10
MEASURED_INVARIANT_TA = 1.2e-10


def measured(scale, ta=False):
    """The six constants (L, beta, Q, gamma, gradient, invariant) of a scale, sweep or Ta."""
    if ta:
        return np.array([MEASURED_L_FIXED_TA if scale == "fixed" else MEASURED_L_TA, MEASURED_BETA_TA, MEASURED_Q_TA,
                         MEASURED_GAMMA_TA, MEASURED_GRAD_TA, MEASURED_INVARIANT_TA])
    return np.array([MEASURED_L_FIXED if scale == "fixed" else MEASURED_L, MEASURED_BETA, MEASURED_Q, MEASURED_GAMMA, MEASURED_GRAD,
                     MEASURED_INVARIANT])


def bars(scale, ta=False):
    """The GPU bars: 10 x the constants."""
    return 10 * measured(scale, ta)


NAMES = ("L", "beta", "Q", "gamma", "grad", "invariant")


# ---- the cases --------------------------------------------------------------------------------------------------------
def own_rows(K, sizes, seed, zero_column=None):
    """Rows built like ``cc.sweep_case``: columns scaled over two decades, weights in [0.5, 2], shuffled, three rows without a
    category; ``sizes``: rows per category."""
    rng = np.random.default_rng(seed)
    cat = np.concatenate([np.full(int(n), i, dtype=np.int32) for i, n in enumerate(sizes)] + [np.full(3, -1, dtype=np.int32)])
    rng.shuffle(cat)
    m = len(cat)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, K)
    A = rng.standard_normal((m, K)) * scale
    truth = rng.standard_normal(K) / scale
    b = A @ truth + 0.1 * rng.standard_normal(m)
    if zero_column is not None:
        A[:, zero_column] = 0.0
    w0 = rng.uniform(0.5, 2.0, m)
    return np.ascontiguousarray(A), b, w0, cat


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, b, w0, category per row, K, C, S (P, C), training (C,) bool) of a case.
    sweep cases: the rows of ``cc.sweep_case`` with category = composite category % 4 (the folds pooled), all training;
    "c9":  K = 31, C = 9: category 5 is a testing category, category 6 is scaled 0 by every candidate and category 2 by candidate
           3 only -- a combine tail of 8 + 1 and a category tile that is partly empty;
    "c17": K = 7, C = 17: a second category tile with one row;  "zerocol": K = 31, C = 4, column 5 identically zero."""
    if name == C9:
        K, C = 31, 9
        A, b, w0, cat = own_rows(K, [K + 13 + c % 3 for c in range(C)], 8109)
        S = cc.ga_scales(P, C, 4243)
        S[:, 6] = 0.0
        S[3, 2] = 0.0
        training = np.ones(C, dtype=bool)
        training[5] = False
        return A, b, w0, cat, K, C, S, training
    if name == C17:
        K, C = 7, 17
        A, b, w0, cat = own_rows(K, [K + 5 + c % 4 for c in range(C)], 8117)
        return A, b, w0, cat, K, C, cc.ga_scales(P, C, 4244), np.ones(C, dtype=bool)
    if name == ZERO:
        K, C = 31, 4
        A, b, w0, cat = own_rows(K, [K + 13 + c for c in range(C)], 8131, zero_column=5)
        return A, b, w0, cat, K, C, cc.ga_scales(P, C, 4245), np.ones(C, dtype=bool)
    A, b, w0, ccat, K = cc.sweep_case(name)
    cat = np.where(ccat >= 0, ccat % cc.SWEEP_C, -1).astype(np.int32)
    return A, b, w0, cat, K, cc.SWEEP_C, cc.sweep_scales(name), np.ones(cc.SWEEP_C, dtype=bool)


def labels(cat, training):
    """(rows kept, fs_dict) under which ``CandidateFits`` builds the categories of a case in the same order: category c is
    (group c // 2, energy | force); a testing category is an odd one, so the sorted keys keep the order."""
    keep = cat >= 0
    c = cat[keep]
    fs = {"Groups": [f"g{int(x) // 2:02d}" for x in c], "Testing": [not bool(training[int(x)]) for x in c],
          "Row_Type": ["Force" if int(x) % 2 else "Energy" for x in c]}
    return keep, fs


def training_blocks(A, b, w0, cat, C, training, blocks=cc.blocks_numpy):
    """The blocks as ``CandidateFits`` holds them: the rows of a testing category are masked out."""
    out = blocks(A, b, w0, cat, C)
    out[~np.asarray(training)] = 0
    return out


def constants(w0, cat, C):
    """(n (C,), sum log|w0| (C,)) over the rows with a category and w0 != 0."""
    keep = (cat >= 0) & (w0 != 0)
    return (np.bincount(cat[keep], minlength=C).astype(np.float64),
            np.bincount(cat[keep], weights=np.log(np.abs(w0[keep])), minlength=C))


def case_alpha(name, ialpha):
    A, b, w0, cat, K, C, S, training = case(name)
    return cc.base_alpha(training_blocks(A, b, w0, cat, C, training), K, cc.ALPHA_FRACTIONS[ialpha])


# ---- oracle R ---------------------------------------------------------------------------------------------------------
def chol_ld(H):
    """The lower Cholesky factor of H in long double."""
    L = np.array(H, dtype=LD)
    n = L.shape[0]
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return np.tril(L)


def tri_inv_ld(L):
    """The inverse of a lower triangle in long double, row by row."""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, i] = 1 / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def evidence_ld(bl, rows, s, alpha, training, n, slw0):
    """Oracle R for one candidate from the long-double blocks ``bl`` (C, K^2 + K + 3) and ``rows`` = (A, b, w0, cat) in long double
    (``None``: Q from the blocks).  Returns a dict: L, grad, gla, sigma2 per scale; beta, logdet, Q, gamma, k, N, R and the error
    scales."""
    C = bl.shape[0]
    K = int(round((np.sqrt(4 * bl.shape[1] - 11) - 1) / 2))
    KK = K * K
    s = np.asarray(s, dtype=LD)
    active = (np.asarray(s) != 0) & training & (n > 0)
    lam = np.where(active, s * s, LD(0))
    G, r, bb = bl[:, :KK].reshape(C, K, K), bl[:, KK:KK + K], bl[:, KK + K]
    H = np.tensordot(lam, G, axes=1)
    live = np.diag(H) != 0
    k = int(live.sum())
    beta = np.zeros(K, dtype=LD)
    Sinv = np.zeros((K, K), dtype=LD)
    logdet = LD(0)
    if k:
        Hl = H[np.ix_(live, live)] + LD(alpha) * np.eye(k, dtype=LD)
        d = np.sqrt(np.diag(Hl))
        Lf = chol_ld(Hl / d[:, None] / d[None, :])
        X = tri_inv_ld(Lf)
        Wi = (X.T @ X) / d[:, None] / d[None, :]
        Sinv[np.ix_(live, live)] = Wi
        beta[live] = Wi @ (lam @ r)[live]
        logdet = 2 * (np.log(np.diag(Lf)).sum() + np.log(d).sum())
    if rows is None:
        Q = bb - 2 * (r @ beta) + np.einsum("i,cij,j->c", beta, G, beta)
    else:
        A, b, w0, cat = rows
        res = (w0 * (b - A @ beta)) ** 2
        Q = np.array([res[cat == c].sum() for c in range(C)], dtype=LD)
    Q = np.where(active, Q, LD(0))
    T = np.einsum("ij,cij->c", Sinv, G)
    gamma = lam * T
    bnorm = beta @ beta
    trinv = np.trace(Sinv)
    N = LD(n[active].sum())
    R = (lam * Q).sum() + LD(alpha) * bnorm
    Np = N if alpha > 0 else N - k
    with np.errstate(divide="ignore"):
        slw = sum((LD(slw0[c]) + LD(n[c]) * np.log(np.abs(s[c])) for c in range(C) if active[c]), LD(0))
    head = slw - logdet / 2 + (LD(k) / 2 * np.log(LD(alpha)) if alpha > 0 else LD(0))
    out = {"beta": beta, "logdet": logdet, "Q": Q, "gamma": gamma, "k": k, "N": N, "Np": Np, "R": R, "active": active,
           "trinv": trinv, "bnorm": bnorm, "lam": lam}
    for scale in SCALES:
        if scale == "fixed":
            sigma2, kappa = LD(1), LD(1)
            L = head - R / 2 - Np / 2 * LOG_2PI
        else:
            sigma2 = R / Np
            kappa = 1 / sigma2
            L = head - Np / 2 * (np.log(sigma2) + 1 + LOG_2PI)
        grad = np.where(active, n - gamma - kappa * lam * Q, LD(0))
        gla = (k - LD(alpha) * trinv - kappa * LD(alpha) * bnorm) / 2 if alpha > 0 else LD(0)
        out[scale] = {"L": L, "sigma2": sigma2, "grad": grad, "gla": gla,
                      "sgrad": np.where(active, n + np.abs(gamma) + kappa * lam * np.abs(Q), LD(0)),
                      "sgla": (k + LD(alpha) * trinv + kappa * LD(alpha) * bnorm) / 2 if alpha > 0 else LD(0)}
    ab = np.abs(beta)
    out["sQ"] = np.where(active, bb + 2 * (np.abs(r) @ ab) + np.einsum("i,cij,j->c", ab, np.abs(G), ab), LD(0))
    out["sgamma"] = np.sqrt((Sinv * Sinv).sum()) * np.sqrt((G * G).sum(axis=(1, 2))) * lam
    return out


def oracle_from(A, b, w0, cat, S, alpha, training):
    """Oracle R of every candidate of S: a list of ``evidence_ld`` dicts."""
    C = S.shape[1]
    bl = training_blocks(A, b, w0, cat, C, training, cc.blocks_ld)
    n, slw0 = constants(w0, cat, C)
    rows = (np.asarray(A, dtype=LD), np.asarray(b, dtype=LD), np.asarray(w0, dtype=LD), cat)
    return [evidence_ld(bl, rows, S[p], alpha, np.asarray(training), n, slw0) for p in range(S.shape[0])]


@functools.lru_cache(maxsize=None)
def oracle(name, ialpha):
    """Oracle R of a case at ``cc.ALPHA_FRACTIONS[ialpha]``, computed once and shared: (alpha, list of dicts)."""
    A, b, w0, cat, K, C, S, training = case(name)
    alpha = case_alpha(name, ialpha)
    return alpha, oracle_from(A, b, w0, cat, S, alpha, training)


def evidence_value_ld(A, b, w0, cat, s, alpha, training):
    """{scale: L} of one candidate in long double from the rows (the function the central differences are taken of)."""
    C = len(s)
    bl = training_blocks(A, b, w0, cat, C, training, cc.blocks_ld)
    n, slw0 = constants(w0, cat, C)
    ref = evidence_ld(bl, None, s, alpha, np.asarray(training), n, slw0)
    return {scale: ref[scale]["L"] for scale in SCALES}


# ---- oracle D ---------------------------------------------------------------------------------------------------------
def density_ld(A, b, w0, cat, s, alpha, training):
    """log N(y; 0, diag(w^-2) + A A' / alpha) over the active rows, w = w0 s[category], in long double."""
    s = np.asarray(s, dtype=np.float64)
    keep = (cat >= 0) & (w0 != 0)
    keep[keep] = (s[cat[keep]] != 0) & np.asarray(training)[cat[keep]]
    Al, y = np.asarray(A[keep], dtype=LD), np.asarray(b[keep], dtype=LD)
    w = np.asarray(w0[keep], dtype=LD) * np.asarray(s, dtype=LD)[cat[keep]]
    N = len(y)
    cov = Al @ Al.T / LD(alpha) + np.diag(1 / (w * w))
    Lf = chol_ld(cov)
    z = y.copy()
    for i in range(N):                                    # L z = y
        z[i] = (z[i] - Lf[i, :i] @ z[:i]) / Lf[i, i]
    return -(z @ z) / 2 - np.log(np.diag(Lf)).sum() - N / LD(2) * LOG_2PI, N


def tiny_case(K):
    """(A, b, w0, cat, s, alpha, training): 3 categories, 40 rows, one row without a category; for oracle D."""
    A, b, w0, cat = own_rows(K, [13, 14, 10], 8200 + K)
    A, b, w0, cat = A[:-2], b[:-2], w0[:-2], cat[:-2]     # 38 rows, some without a category
    s = np.array([0.7, -1.9, 3.1])
    return A, b, w0, cat, s, 0.37, np.ones(3, dtype=bool)


# ---- the measured quantities ------------------------------------------------------------------------------------------
def f64(x):
    return np.asarray(x, dtype=np.float64)


def ratio(err, scale):
    """max err / scale over the entries with a scale; entries whose scale is 0 must be met exactly."""
    err, scale = np.atleast_1d(f64(err)), np.atleast_1d(f64(scale))
    assert np.all(err[scale == 0] == 0), (err, scale)
    return float(np.max(err[scale > 0] / scale[scale > 0])) if np.any(scale > 0) else 0.0


def errors(ref, ev, S, alpha, n, against=None):
    """(L, beta, Q, gamma, gradient, invariant) errors of a ``CandidateEvidence`` against the list of oracle dicts ``ref`` -- or,
    with ``against`` (another ``CandidateEvidence``), its differences from that one in the oracle's units (invariant: 0)."""
    scale = ev.scale
    k = np.zeros(6)
    for p, r in enumerate(ref):
        o = r[scale]
        assert ev.status[p] == 0 and ev.live[p] == r["k"], (p, ev.status[p], ev.live[p], r["k"])
        assert np.array_equal(ev.active[p], r["active"])
        if against is None:
            want = (o["L"], r["beta"], r["Q"], r["gamma"], o["grad"], o["gla"])
        else:
            want = tuple(LD(1) * getattr(against, f)[p] for f in ("log_evidence", "beta", "rss", "dof", "grad_logS", "grad_logalpha"))
        kl = abs(float(LD(ev.log_evidence[p]) - want[0])) / float(r["N"])
        bn = float(np.sqrt(r["bnorm"]))
        kb = float(np.linalg.norm(f64(LD(1) * ev.beta[p] - want[1]))) / bn if bn > 0 else 0.0
        kq = ratio(np.abs(LD(1) * ev.rss[p] - want[2]), r["sQ"])
        kg = ratio(np.abs(LD(1) * ev.dof[p] - want[3]), r["sgamma"])
        kd = max(ratio(np.abs(LD(1) * ev.grad_logS[p] - want[4]), o["sgrad"]),
                 ratio(np.abs(LD(1) * ev.grad_logalpha[p] - want[5]), o["sgla"]))
        k = np.maximum(k, (kl, kb, kq, kg, kd, invariants(r, ev, p, S[p], alpha) if against is None else 0.0))
    return k


def invariants(r, ev, p, s, alpha):
    """The worse of the two invariants of candidate p, each over the sum of the magnitudes that enter it (oracle R's)."""
    o = r[ev.scale]
    kappa = 1.0 / ev.sigma2[p]
    bnorm = float(ev.beta[p] @ ev.beta[p])
    # sum_c gamma_c + alpha tr(S^-1) = k, with alpha tr(S^-1) = k - 2 dL/dlog alpha - kappa alpha |beta|^2 read back
    if alpha > 0:
        one = abs(ev.dof[p].sum() - 2 * ev.grad_logalpha[p] - kappa * alpha * bnorm)
    else:
        one = abs(ev.dof[p].sum() - ev.live[p])
    one /= max(float(np.abs(r["gamma"]).sum() + 2 * o["sgla"]), float(r["k"]), 1.0)
    target = 0.0 if ev.scale == "profiled" else float(r["Np"] - r["R"])
    two = abs(ev.grad_logS[p].sum() + 2 * ev.grad_logalpha[p] - target) / float(o["sgrad"].sum() + 2 * o["sgla"] + abs(target))
    return max(float(one), float(two))


def host_result(name, ialpha, scale):
    A, b, w0, cat, K, C, S, training = case(name)
    n, slw0 = constants(w0, cat, C)
    return ce.host_evidence(training_blocks(A, b, w0, cat, C, training), S, case_alpha(name, ialpha), n, slw0, training, K, scale)


# ---- the Ta golden case ----------------------------------------------------------------------------------------------
TA_P = cc.TA_P + 1


@functools.lru_cache(maxsize=None)
def ta_case():
    """(A, b, w0 = 1, category per row, keys, S (9, C), training): the golden rows with the categories of ``CandidateFits``, the
    eight GA-style candidates of ``cc.ta_layout`` and one whose scales are ``gc.TA_WEIGHTS`` by row type."""
    golden = os.path.join(ROOT, "tests", "golden")
    z, fits = np.load(os.path.join(golden, "ta_abw.npz")), dict(np.load(os.path.join(golden, "ta_reference_fits.npz")))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    cat, keys, _, _, S = cc.ta_layout(cc.ta_labels(fits))
    S = np.vstack([S, [gc.TA_WEIGHTS[k[2]] for k in keys]])
    return A, b, np.ones(len(b)), cat, keys, S, np.array([not k[1] for k in keys], dtype=bool)


@functools.lru_cache(maxsize=None)
def ta_oracle(name):
    A, b, w0, cat, keys, S, training = ta_case()
    return oracle_from(A, b, w0, cat, S, cc.TA_ALPHAS[name], training)


def ta_host(name, scale):
    A, b, w0, cat, keys, S, training = ta_case()
    C = len(keys)
    n, slw0 = constants(w0, cat, C)
    return ce.host_evidence(training_blocks(A, b, w0, cat, C, training), S, cc.TA_ALPHAS[name], n, slw0, training, A.shape[1], scale)


def measure():
    """Prints what the MEASURED_* constants record."""
    def report(worst, tag):
        both = np.maximum(worst["profiled"], worst["fixed"])
        print(f"MEASURED_L{tag} = {worst['profiled'][0]:.1e}  MEASURED_L_FIXED{tag} = {worst['fixed'][0]:.1e}  "
              + "  ".join(f"MEASURED_{nm.upper()}{tag} = {v:.1e}" for nm, v in list(zip(NAMES, both))[1:]))

    worst = {scale: np.zeros(6) for scale in SCALES}
    for name in CASES:
        A, b, w0, cat, K, C, S, training = case(name)
        n, _ = constants(w0, cat, C)
        for ia in range(len(cc.ALPHA_FRACTIONS)):
            alpha, ref = oracle(name, ia)
            for scale in SCALES:
                ev = host_result(name, ia, scale)
                k = errors(ref, ev, S, alpha, n)
                print(f"{name:>7s} alpha {alpha:.2e} {scale:8s} " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(NAMES, k))
                      + f"  min pivot {ev.min_pivot.min():.2e}", flush=True)
                worst[scale] = np.maximum(worst[scale], k)
    report(worst, "")
    worst = {scale: np.zeros(6) for scale in SCALES}
    A, b, w0, cat, keys, S, training = ta_case()
    n, _ = constants(w0, cat, len(keys))
    for name in cc.TA_ALPHAS:
        ref = ta_oracle(name)
        for scale in SCALES:
            ev = ta_host(name, scale)
            k = errors(ref, ev, S, cc.TA_ALPHAS[name], n)
            print(f"Ta {name:5s} {scale:8s} " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(NAMES, k))
                  + f"  min pivot {ev.min_pivot.min():.2e}", flush=True)
            worst[scale] = np.maximum(worst[scale], k)
    report(worst, "_TA")


if __name__ == "__main__":
    measure()
