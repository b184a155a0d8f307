"""Inputs, long-double reference, a-priori bars and a faulty float64 mirror for the blocked device Cholesky chain of
fsnap_chol.hip (kernels 8a-8f, the probe Gram and the factor-only form), shared by tests/test_chol_cases_cpu.py and
tests/test_gpu_chol.py.  Pure numpy / scipy, no GPU.

Notation: M = G + alpha I, D = diag(M)^-1/2, H = D M D (unit diagonal), g = D c, z = D^-1 beta, n = K, np = K padded to 64,
eps = 2^-52 (``numpy.finfo(float).eps``, the library's ``numeric_limits<double>::epsilon()``).

Families (``family``): every one returns (G, c) in float64 with column scales spread over decades, so that a solve without
the Jacobi scaling of kernel 8a has no chance.
  gauss         X^T X of (2K + 37) x K Gaussian rows times 10^U(-3, 3) per column; H has kappa ~ 20-30, pivots ~ 0.5
  gauss_wide    the same with 10^U(-8, 8): the statistics span more than 30 decades
  spectrum(k)   S Q diag(k^(-i / (K - 1))) Q^T S, Q from a QR of a Gaussian matrix, S = diag(10^U(-3, 3)); k = 1e2, 1e3, 3e4
                are systems the device answers (smallest pivot above the acceptance threshold 1e-3 of fsnap_solve_device),
                k = 1e6 is one it refuses
  hidden(b)     the generator of tests/test_gpu_condest.py (the identity with I - triu(ones, 1) mixed into the last b
                columns), b = 10, 14: pivots of 0.04-0.07 hide lambda_min = 4e-6 / 2e-8
  dup           gauss with the last column a copy of column 7 (singular: the device must refuse it)

Reference (``reference``): beta_ref by iterative refinement in ``np.longdouble`` (64-bit mantissa) -- a float64 Cholesky
of H as preconditioner, the residual c - M beta in long double, until the scaled correction stops shrinking (at most 12
steps; the error then sits at the long-double rounding level kappa 1e-19, many decades below every bar).  From the float64 H
also lambda_min, kappa_2 and the smallest Cholesky pivot.  Cached per (family, K, alpha).

Bars: inputs and reference only, never the kernel's output.
  backward   r = D (c - M beta_hat), formed in long double;  |r_i| <= bar_i = 4 (3 np + 1) eps (|z_ref|_1 + |g_i|).
             A Cholesky solve satisfies (H + dH) z_hat = g with |dH| <= gamma_{3n+1} |U^T| |U| (Higham, Accuracy and
             Stability of Numerical Algorithms, theorem 10.4), so |g - H z_hat|_i <= gamma_{3n+1} sum_j (|U^T||U|)_ij |z_hat_j|;
             for a unit diagonal (|U^T||U|)_ij <= |u_i| |u_j| = 1 (columns of U have unit norm), which gives
             gamma_{3n+1} |z|_1.  The three roundings of the scaling (H_ij = G_ij d_i d_j, g_i = c_i d_i, beta_i = z_i d_i)
             each add O(eps) of the same form (|H||z| <= |z|_1, and eps |g_i|): the 4 covers those and gamma against n eps.
             The substitutions of kernels 8c and 8e multiply by explicit inverses of the 16 x 16 diagonal blocks, which is
             outside the textbook bound: the mirror below does the same, and tests/test_chol_cases_cpu.py shows how much room
             that leaves (it prints mirror / bar for every case).
  forward    gauss* and spectrum only: |D^-1 (beta_hat - beta_ref)|_2 <= |bar|_2 / lambda_min(H)  (z_hat - z = H^-1 r).
             For hidden this exceeds |z| and says nothing: the backward bar alone applies there (``has_forward``).
  estimate   the probes are a pure integer hash (``probe_values``, a port of fsnap::chol_probe_value): with B the K x 31
             probe matrix, Z = U^-T B and theta = lambda_max(Z^T Z, B^T B), est_ref = (1 / theta) min(1, 120 / K).  The
             device's estimate equals it within 4 (3 np + 1) eps kappa_2(H) relative (theta is a Rayleigh quotient of H^-1:
             a backward error dH of the factor moves it by kappa |dH|), and independently lambda_min / 4 <= est <= 10 lambda_min
             (tests/test_chol_cases_cpu.py checks the band on est_ref for every case the GPU file runs).

Mirror (``mirror``): a float64 numpy model of the shipped algorithm -- padding with an identity block, 64-row panels,
16 x 16 diagonal blocks factorised by rank-1 steps with Y_b = U_bb^-1 from the same row operations on an identity tile, row
tails X_b = Y_b^T (S_b - sum L_bb' X_b'), trailing update with the 32-column strip (right-hand side + 31 probes) carried
along, the last panel's strip rows substituted separately, back substitution in macro-blocks of four panels from the bottom
with x_b = Y_b v_b, beta = D x; ``rhs=`` runs the forward sweep of kernel 8f on the factor instead.  ``FAULTS`` are the
switchable mistakes; tests/test_chol_cases_cpu.py shows that the clean mirror stays within 1.0 bars and that every fault
lands more than 100 bars outside."""
import functools
import types

import numpy as np
import scipy.linalg as sl

LD = np.longdouble
EPS = float(np.finfo(float).eps)
NB, XS, NPROBE, MACRO = 64, 32, 31, 4
ACCEPT_PIVOT = 1.0e-3                    # fsnap_solve_device_rhs: the device answer stands when every pivot is above this

# ---- shapes of the GPU file -----------------------------------------------------------------------------------------------
# 3 to 13 panels, every panel count modulo 4 (the top macro-block of the back substitution has 1, 2, 3 or 4 panels), K modulo
# 64 in {0, 1, 17, 63, ...}; below 232 only with device_solve = 1
K_SWEEP = (129, 145, 160, 191, 192, 193, 232, 255, 256, 257, 319, 320, 321, 337, 383, 384, 385, 447, 448, 449, 512, 513, 576,
           577, 640, 641, 704, 768, 832)
K_MOD4 = (257, 321, 447, 512)            # 5, 6, 7, 8 panels: one K per panel count modulo 4
K_RHS = (129, 192) + K_MOD4              # 3 panels (one partial macro-block) as well
K_LARGE = (1000, 1595)
K_CPU = (129, 192, 257, 384, 448, 640)
SWEEP_FAMILIES = ("gauss", "spectrum3e4")
OTHER_FAMILIES = ("gauss_wide", "spectrum1e2", "spectrum1e3", "hidden10", "hidden14")
ACCEPTED = SWEEP_FAMILIES + OTHER_FAMILIES
REFUSED = ("spectrum1e6", "dup")
ALPHAS = (1.0e-8, 1.0e12)                # times the largest diagonal entry; at 1e12 H is I to rounding
DEVICE_MIN_K = 232                       # fsnap::DEVICE_CHOL_MIN_K: below it the device factorises only on request
LSTSQ_K = (384, 385, 400, 449, 513, 640)  # factor-only form: K16 == np at 384, 640; K16 != np at 385, 400, 449, 513


def pad(K, to=NB):
    return (K + to - 1) // to * to


def panels(K):
    return pad(K) // NB


def top_block(K):
    """Panels in the top (last solved, possibly partial) macro-block of the back substitution."""
    p = panels(K)
    return p % MACRO or MACRO


def probe_values(rows, p):
    """fsnap::chol_probe_value(row, p) of fsnap_chol.hip for an array of rows: 32-bit integer hash -> +-[0.25, 1)."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.asarray(rows, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(p) * np.uint64(0x85EBCA77) + np.uint64(0x27D4EB2F)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & m
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & m
    x ^= x >> np.uint64(15)
    mag = 0.25 + 0.75 * ((x & np.uint64(0xFFFF)).astype(np.float64) / 65536.0)
    return np.where((x & np.uint64(0x10000)) != 0, -mag, mag)


def probe_matrix(K):
    return np.stack([probe_values(np.arange(K), p) for p in range(1, NPROBE + 1)], axis=1)


def gen_eig_max(A, N):
    """Largest eigenvalue of A x = theta N x, N positive definite (both symmetric)."""
    L = np.linalg.cholesky(N)
    W = sl.solve_triangular(L, sl.solve_triangular(L, A, lower=True).T, lower=True)
    return float(np.linalg.eigvalsh(0.5 * (W + W.T))[-1])


# ---- families -------------------------------------------------------------------------------------------------------------

def _seed(name, K):
    return [sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), K]


def hidden_rows(K, m, rng, block):
    """tests/test_gpu_condest.py::hidden with ``block``."""
    M = np.eye(K)
    M[K - block:, K - block:] = np.eye(block) - np.triu(np.ones((block, block)), 1)
    return rng.standard_normal((m, K)) @ M


@functools.lru_cache(maxsize=4)
def family(name, K):
    """Namespace (G, c, rows, y): the K x K statistics of the family, float64, G exactly symmetric; for the families made of rows
    also the rows and the targets y behind c = rows^T y (None otherwise)."""
    rng = np.random.default_rng(_seed(name, K))
    decades = 8.0 if name == "gauss_wide" else 3.0
    s = 10.0 ** rng.uniform(-decades, decades, K)
    rows = y = None
    if name in ("gauss", "gauss_wide", "dup"):
        rows = rng.standard_normal((2 * K + 37, K)) * s
        if name == "dup":
            rows[:, K - 1] = rows[:, 7]
        G = rows.T @ rows
        y = rng.standard_normal(rows.shape[0])
        c = rows.T @ y
    elif name.startswith("hidden"):
        rows = hidden_rows(K, 6000, rng, int(name[6:])) * s
        G = rows.T @ rows
        y = rows @ (rng.standard_normal(K) / s) + 1.0e-3 * rng.standard_normal(rows.shape[0])
        c = rows.T @ y
    elif name.startswith("spectrum"):
        kappa = float(name[8:])
        lam = kappa ** (-np.arange(K) / (K - 1.0))
        for _ in range(16):
            Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
            P = (Q * lam) @ Q.T
            dp = 1.0 / np.sqrt(np.diag(P))
            # kappa = 3e4 sits next to the acceptance threshold (smallest pivot 1.7e-3 ... 3.5e-3 over draws of Q): Q is drawn
            # again until the float64 pivot clears 2.2e-3, so that "accepted" does not hang on the device's last bits
            if kappa != 3.0e4 or np.min(np.diag(np.linalg.cholesky(P * dp[:, None] * dp[None, :]))) ** 2 >= 2.2 * ACCEPT_PIVOT:
                break
        G = P * s[:, None] * s[None, :]
        c = G @ (rng.standard_normal(K) / s) + 1.0e-3 * s * rng.standard_normal(K)
    else:
        raise ValueError(name)
    G = np.triu(G) + np.triu(G, 1).T
    for a in (G, c):
        a.setflags(write=False)
    return types.SimpleNamespace(G=G, c=c, rows=rows, y=y)


def packed(G, c):
    """[G | c | 3 scalars]: the layout fsnap_solve_device reads."""
    return np.concatenate([G.ravel(), c, np.zeros(3)])


# ---- reference ------------------------------------------------------------------------------------------------------------

def refine(ref, c):
    """Solution of M beta = c in long double by iterative refinement, preconditioned with the float64 Cholesky factor of H."""
    cl = np.asarray(c, dtype=LD)
    beta = np.zeros(ref.K, dtype=LD)
    last = np.inf
    for _ in range(12):
        r = cl - ref.M @ beta
        dz = sl.cho_solve((ref.U, False), (ref.d * r).astype(np.float64))
        size = float(np.linalg.norm(dz))
        if not size < last:
            break
        beta = beta + ref.d.astype(LD) * dz.astype(LD)
        last = size
    return beta


def bars(ref, c, beta_ref):
    """(bar vector of the backward check, bar of the forward check) for the right-hand side c."""
    z1 = float(np.sum(np.abs(beta_ref / ref.d.astype(LD))))
    bar = 4.0 * (3 * ref.np + 1) * EPS * (z1 + np.abs(np.asarray(c) * ref.d))
    return bar, float(np.linalg.norm(bar)) / ref.lam_min


@functools.lru_cache(maxsize=3)
def reference(name, K, alpha_rel=0.0):
    """Everything the bars need for (family, K, alpha = alpha_rel x the largest diagonal entry of G)."""
    fam = family(name, K)
    G, c = fam.G, fam.c
    alpha = float(alpha_rel * np.max(np.diag(G)))
    ref = types.SimpleNamespace(name=f"{name}-K{K}" + (f"-a{alpha_rel:g}" if alpha_rel else ""), family=name, K=K, np=pad(K),
                                G=G, c=c, rows=fam.rows, y=fam.y, alpha=alpha, has_forward=not name.startswith("hidden"))
    ref.M = G.astype(LD)
    ref.M[np.diag_indices(K)] += LD(alpha)
    ref.d = 1.0 / np.sqrt(np.diag(G) + alpha)
    H = (G + alpha * np.eye(K)) * ref.d[:, None] * ref.d[None, :]
    H[np.diag_indices(K)] = 1.0
    ref.H = H
    w = np.linalg.eigvalsh(H)
    ref.lam_min, ref.kappa = float(w[0]), float(w[-1] / w[0]) if w[0] > 0 else np.inf
    try:
        ref.U = np.linalg.cholesky(H).T
        ref.pivot = float(np.min(np.diag(ref.U)) ** 2)
    except np.linalg.LinAlgError:
        ref.U, ref.pivot = None, 0.0
    if ref.U is not None:
        ref.beta = refine(ref, c)
        ref.bar, ref.fwd_bar = bars(ref, c, ref.beta)
        B = probe_matrix(K)
        Z = sl.solve_triangular(ref.U, B, trans="T")
        ref.theta = gen_eig_max(Z.T @ Z, B.T @ B)
        ref.est = (1.0 / ref.theta) * min(1.0, 120.0 / K)
        ref.est_bar = 4.0 * (3 * ref.np + 1) * EPS * ref.kappa
    return ref


def reference_rhs(ref, c):
    """(beta_ref, bar, forward bar) of one more right-hand side for the matrix of ``ref``."""
    beta = refine(ref, c)
    return (beta,) + bars(ref, c, beta)


# ---- scores (error / bar) -------------------------------------------------------------------------------------------------

def backward(ref, beta_hat, c=None, bar=None):
    c = ref.c if c is None else c
    bar = ref.bar if bar is None else bar
    if not np.all(np.isfinite(beta_hat)):
        return np.inf
    r = ref.d.astype(LD) * (np.asarray(c, dtype=LD) - ref.M @ np.asarray(beta_hat, dtype=LD))
    return float(np.max(np.abs(r) / bar))


def forward(ref, beta_hat, beta_ref=None, fwd_bar=None):
    beta_ref = ref.beta if beta_ref is None else beta_ref
    fwd_bar = ref.fwd_bar if fwd_bar is None else fwd_bar
    if not np.all(np.isfinite(beta_hat)):
        return np.inf
    e = (np.asarray(beta_hat, dtype=LD) - beta_ref) / ref.d.astype(LD)
    return float(np.sqrt(np.sum(e * e))) / fwd_bar


def estimate(ref, est):
    if not np.isfinite(est) or est <= 0.0:
        return np.inf
    return abs(est / ref.est - 1.0) / ref.est_bar


def in_band(ref, est):
    """The design's claim about the estimate."""
    return ref.lam_min / 4.0 <= est <= 10.0 * ref.lam_min


def score(ref, beta_hat, est=None, c=None, rhs_ref=None):
    """Dict of error / bar: 'bwd', 'fwd' (where the family has a forward bar), 'est' (when an estimate is given)."""
    if rhs_ref is None:
        out = {"bwd": backward(ref, beta_hat)}
        if ref.has_forward:
            out["fwd"] = forward(ref, beta_hat)
    else:
        beta_ref, bar, fwd_bar = rhs_ref
        out = {"bwd": backward(ref, beta_hat, c, bar)}
        if ref.has_forward:
            out["fwd"] = forward(ref, beta_hat, beta_ref, fwd_bar)
    if est is not None:
        out["est"] = estimate(ref, est)
    return out


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.array_equal(x.view(np.uint64), y.view(np.uint64)))


# ---- mirror ---------------------------------------------------------------------------------------------------------------
# what each fault breaks; the last column says where it applies
FAULTS = {
    "skip_trailing_tile": "one 16 x 16 tile of the first panel's trailing update is not applied",
    "raw_last_strip": "the strip rows of the last panel are left raw (no forward substitution behind the last panel)",
    "skip_top_offdiag": "the block right of the diagonal block is skipped in a PARTIAL top macro-block of the back substitution",
    "zero_padding": "the padding carries zeros instead of an identity block",
    "rsq_no_newton": "one pivot reciprocal keeps the 2^-23 relative error of v_rsq_f64 (no Newton step)",
    "beta_not_unscaled": "one beta_j is handed out as x_j, without the factor d_j",
    "stale_x": "the back substitution reads the x slot of the panel before the previous one",
}
# A lost SECOND Newton step leaves 1.5 (2^-23)^2 ... = 3e-14 relative in one pivot reciprocal: 3e-14 |U_j.| in one row of
# the factor is below the bars (4 (3 np + 1) eps |z|_1 is 5e-13 |z|_1 at np = 192 and grows with np) -- the bars cannot
# see it and no test here claims to.


def applicable(K, fault):
    if fault == "zero_padding":
        return K % NB != 0
    if fault == "skip_top_offdiag":
        return 2 <= top_block(K) < MACRO
    return True


def _substitute_T(U11, v):
    """y = U11^-T v by plain substitution (reciprocal of the diagonal, one step per row), as kernels 8e / 8f / probe do."""
    v = np.array(v, dtype=np.float64)
    invd = 1.0 / np.diag(U11)
    for k in range(U11.shape[0]):
        v[k] = v[k] * invd[k]
        v[k + 1:] -= U11[k, k + 1:, None] * v[k] if v.ndim == 2 else U11[k, k + 1:] * v[k]
    return v


def _diag_block(T, bad_pivot):
    """The 64 x 64 diagonal block as the four-wave pipeline factorises it: per 16-block a, sixteen rank-1 steps on the rows of
    the block across the strips c >= a (and on an identity tile: Y_a = U_aa^-1), then T_bc -= U_ab^T U_ac for the blocks below."""
    T = T.copy()
    Y = np.zeros((4, 16, 16))
    pmin = np.inf
    for a in range(4):
        lo, hi = 16 * a, 16 * a + 16
        Z = np.eye(16)
        for j in range(lo, hi):
            piv = T[j, j]
            pmin = min(pmin, piv) if piv == piv else np.nan
            with np.errstate(all="ignore"):
                inv = 1.0 / np.sqrt(piv)
            if j == bad_pivot:
                inv *= 1.0 + 2.0 ** -23
            T[j, j:] *= inv
            Z[j - lo] *= inv
            mult = T[j, j + 1:hi]
            T[j + 1:hi, j + 1:] -= mult[:, None] * T[j, j + 1:]
            Z[j - lo + 1:] -= mult[:, None] * Z[j - lo]
        Y[a] = Z.T
        T[hi:, hi:] -= T[lo:hi, hi:].T @ T[lo:hi, hi:]
    return np.triu(T), Y, pmin


def mirror(G, c, alpha=0.0, fault=None, rhs=None):
    """float64 model of launch_chol_large (and, with ``rhs``, of launch_chol_resolve on its factor).
    Returns a namespace: beta, pivot (smallest), est (lambda_min estimate of the probes)."""
    n = G.shape[0]
    np_ = pad(n)
    npanel = np_ // NB
    with np.errstate(all="ignore"):
        d = 1.0 / np.sqrt(np.diag(G) + alpha)
        W = np.zeros((np_, np_ + XS))
        W[:n, :n] = ((G + alpha * np.eye(n)) * d[:, None]) * d[None, :]
        if fault != "zero_padding":
            W[np.arange(n, np_), np.arange(n, np_)] = 1.0
        B = probe_matrix(n)
        W[:n, np_] = np.asarray(c) * d
        W[:n, np_ + 1:] = B
        Uf = np.zeros_like(W)
        Yall = np.zeros((npanel, 4, 16, 16))
        pivot = np.inf
        for p in range(npanel):
            jb, je = NB * p, NB * p + NB
            bad = 3 if (fault == "rsq_no_newton" and p == 0) else -1
            U11, Yall[p], pm = _diag_block(W[jb:je, jb:je], bad)
            pivot = min(pivot, pm) if pm == pm else np.nan
            Uf[jb:je, jb:je] = U11
            if je == np_:
                break
            # row tails of the panel, all columns right of it and the strip: X_b = Y_b^T (S_b - sum_b' L_bb' X_b')
            X = W[jb:je, je:].copy()
            for b in range(4):
                acc = X[16 * b:16 * b + 16].copy()
                for bp in range(b):
                    acc -= U11[16 * bp:16 * bp + 16, 16 * b:16 * b + 16].T @ X[16 * bp:16 * bp + 16]
                X[16 * b:16 * b + 16] = Yall[p, b].T @ acc
            Uf[jb:je, je:] = X
            upd = X[:, :np_ - je].T @ X
            if fault == "skip_trailing_tile" and p == 0:
                upd[16:32, 32:48] = 0.0
            W[je:, je:] -= upd
        # the strip of the last panel: raw in the work matrix, substituted by the back substitution / the probe kernel
        r0 = np_ - NB
        last = W[r0:, np_:] if fault == "raw_last_strip" else _substitute_T(Uf[r0:, r0:np_], W[r0:, np_:])
        strip = np.vstack([Uf[:r0, np_:], last])
        zv = strip[:, 0].copy()
        if rhs is not None:
            # kernel 8f: forward sweep of one more right-hand side with the factor
            zv = np.zeros(np_)
            zv[:n] = np.asarray(rhs) * d
            for p in range(npanel):
                jb, je = NB * p, NB * p + NB
                zv[jb:je] = _substitute_T(Uf[jb:je, jb:je], zv[jb:je])
                zv[je:] -= Uf[jb:je, je:np_].T @ zv[jb:je]
        # back substitution in macro-blocks of four panels from the bottom
        hi = npanel
        while hi > 0:
            lo = max(hi - MACRO, 0)
            partial_top = lo == 0 and hi - lo < MACRO
            xs = {}
            for pb in range(hi - 1, lo - 1, -1):
                jb, je = NB * pb, NB * pb + NB
                v = zv[jb:je].copy()
                if pb + 1 < hi:
                    xp = xs[pb + 1]
                    if fault == "stale_x":
                        xp = xs.get(pb + 2, np.zeros(NB))
                    if not (fault == "skip_top_offdiag" and partial_top):
                        v -= Uf[jb:je, je:je + NB] @ xp
                    # the other waves, one panel behind: the rows of the macro-block above this panel
                    zv[NB * lo:jb] -= Uf[NB * lo:jb, je:je + NB] @ xs[pb + 1]
                for b in range(3, -1, -1):
                    xb = Yall[pb, b] @ v[16 * b:16 * b + 16]
                    v[16 * b:16 * b + 16] = xb
                    v[:16 * b] -= Uf[jb:jb + 16 * b, jb + 16 * b:jb + 16 * b + 16] @ xb
                xs[pb] = v
                zv[jb:je] = v
            if lo > 0:
                zv[:NB * lo] -= Uf[:NB * lo, NB * lo:NB * hi] @ zv[NB * lo:NB * hi]
            hi = lo
        beta = zv[:n] * d
        if fault == "beta_not_unscaled":
            beta[n // 3] = zv[n // 3]
        Z = strip[:, 1:]
        est = np.nan
        if np.all(np.isfinite(Z)):
            theta = gen_eig_max(Z.T @ Z, B.T @ B)
            est = (1.0 / theta) * min(1.0, 120.0 / n) if theta > 0 else 0.0
    return types.SimpleNamespace(beta=beta, pivot=float(pivot), est=float(est))


# ---- rows of the factor-only cases (fsnap_lstsq_rows from 384 columns on) ---------------------------------------------------

def conditioned(m, K, kappa, mode, seed):
    """m x K rows with singular values 1 ... 1 / kappa ('geometric') or all 1 but the last ('one')."""
    r = np.random.default_rng(seed)
    U, _ = np.linalg.qr(r.standard_normal((m, K)))
    V, _ = np.linalg.qr(r.standard_normal((K, K)))
    if mode == "geometric":
        s = np.logspace(0, -np.log10(kappa), K)
    else:
        s = np.ones(K)
        s[-1] = 1.0 / kappa
    return (U * s) @ V.T
