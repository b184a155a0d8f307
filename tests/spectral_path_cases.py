"""Cases, oracles and bars of the grouped K-fold spectral paths (tests/test_spectral_path_cpu.py,
tests/test_gpu_spectral_path.py): generators and oracles only.

Every case plants its spectrum.  The weighted rows are U diag(s) W^T D with orthonormal U, orthogonal W, singular values s in
[0.7, 1] and the bad column scalings D_jj = 10^+2 (head columns) or 10^-2 (tail columns, every fourth): D M D with a
well-conditioned M has one cluster of eigenvalues per scaling, a head near 1e4 and a tail near 1e-4, 1e8 / kappa(M) apart -- the
planted gap -- while the diagonally scaled matrix keeps kappa(M) <= 4 (the Demmel-Veselic case).  Variants of the K = 31 case: a
duplicated column (rank K - 1), a column touched by one fold only (dead in that refit), a fold without rows.  The layout is
tests/ard_path_cases.py's sweep: F = 3 folds of about 3 K + 40 rows, row classes i mod 3.

Oracle A (no truncation active): the long-double Cholesky refit (Qm + alpha I) beta = qv on the live columns of the float64
downdated system, the rowwise long-double held-out sums per class and the rowwise long-double training sse.  Oracle B (any
setting): ``scipy.linalg.eigh`` of the same float64 system with the sums carried in long double.  Oracle C:
``spectral_path.spectral_path_host``.

ADMISSION is a condition on oracle B alone, asserted before anything is compared (``admit``): every eigenvalue of every
problem is at least a factor 1 +- 1e-6 away from the cut of every setting, and wherever a setting drops a direction the kept
set lies a factor >= 1e3 above the dropped one.  After admission ranks and supports must EQUAL oracle B's.

BARS.  Errors follow c n_live eps lambda_max / (smallest kept lambda + alpha), relative in the sqrt(diag Qm)-weighted norm.
``python tests/spectral_path_cases.py`` measures the HOST route against oracles A / B over all cases and writes
profiles/spectral_path_accuracy.txt; the constants below are that file's worst ratios.  The kernel is allowed 4 x the host's
worst against the oracles and 2 x that against the host (two correct Jacobi runs round differently); neither constant comes
from a kernel's output.
"""
import functools
import os
import sys

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fitsnap_amd.solvers import folds as ff  # noqa: E402
from fitsnap_amd.solvers import spectral_path as sp  # noqa: E402
from candidate_cv_cases import blocks_numpy, chol_solve_ld  # noqa: E402,F401

LD = np.longdouble
EPS = np.finfo(np.float64).eps

SWEEP_K = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 143, 144]   # byes (odd n), wave, LDS and register edges
LDS_EDGE_K = [113, 114]                      # kernel E1 keeps the eigenvectors in LDS up to 113 columns (155 KiB), in scratch from 114
GRAM_K = [1, 2, 3, 17, 31, 64, 144]
SWEEP_F, NCLASS = 3, 3
ALPHA_FRACTIONS = (0.0, 1e-8, 1e-2)          # alpha = fraction x lambda_max of the total
CUT_MARGIN, GAP = 1e-6, 1e3                  # the admission

# Measured by ``python tests/spectral_path_cases.py`` (profiles/spectral_path_accuracy.txt): the host route's worst ratios,
# each rounded UP to two digits
#   MEASURED_COEF    scaled coefficient error / (n_live eps lambda_max / (smallest kept lambda + alpha)), against A and B
#   MEASURED_EIG     |lambda - lambda_B| / (n_live eps lambda_max)
#   MEASURED_EIG_REL |lambda / lambda_ref - 1| / (n_live eps) on the well-scaled (sweep) cases, against long-double Jacobi (eig_ld)
#   MEASURED_SCALAR  |dof - dof_B| and |sse - sse_ref| / y2 over (n_live eps lambda_max / (smallest kept lambda + alpha))
#   MEASURED_HELD    |h - rowwise long double| / (eps (bb + 2 |beta| . |c| + |beta|^T |G| |beta|))
# The duplicated-column case has its own coefficient constant: its float64 matrix has an EXACT zero eigenvalue, whose
# eigenvector LAPACK (oracle B) resolves to eps lambda_max / (tail lambda) only, and that error is what the ratio shows.
MEASURED_COEF = 2.8
MEASURED_COEF_DUP = 6.1e+01
MEASURED_EIG = 8.8e-01
MEASURED_EIG_REL = 3.4e-01
MEASURED_SCALAR = 1.1
MEASURED_HELD = 1.8
ORACLE_FACTOR, HOST_FACTOR = 4.0, 8.0        # kernel against the oracles; against the host route (2 x again)


def planted_rows(seed, K, sizes, dup=None, lone=None):
    """(A, b, w, fold, cls): the weighted rows are U diag(s) W^T D (see the module text).  ``dup`` = (j, i): column j repeats
    column i; ``lone`` = (j, f): column j is zero outside fold f."""
    rng = np.random.default_rng(seed)
    m = int(sum(sizes))
    U = np.linalg.qr(rng.standard_normal((m, K)))[0]
    W = np.linalg.qr(rng.standard_normal((K, K)))[0]
    s = np.linspace(1.0, 0.7, K)
    D = np.where(np.arange(K) % 4 == 1, 1e-2, 1e2)
    X = (U * s) @ W.T * D
    w = rng.uniform(0.5, 2.0, m)
    truth = rng.standard_normal(K) / D
    y = X @ truth + 0.1 * rng.standard_normal(m)
    A, b = X / w[:, None], y / w
    fold = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    cls = (np.arange(m) % NCLASS).astype(np.uint8)
    if dup is not None:
        A[:, dup[0]] = A[:, dup[1]]
    if lone is not None:
        A[fold != lone[1], lone[0]] = 0.0
    return np.ascontiguousarray(A), b, w, fold, cls


def sizes_of(K):
    return [3 * K + 40, 3 * K + 41, 3 * K + 39]


VARIANTS = {"dup": dict(dup=(7, 2)), "lone": dict(lone=(5, 1)), "empty": dict()}


@functools.lru_cache(maxsize=None)
def case(name, nsub=1):
    """(A, b, w, fold, cls, blocks, K, F, alphas, rconds) of case ``name``: an int K of the sweep, or a variant of K = 31."""
    if name in VARIANTS:
        K = 31
        sizes = sizes_of(K) + ([0] if name == "empty" else [])
        A, b, w, fold, cls = planted_rows(7000 + len(name), K, sizes, **VARIANTS[name])
    else:
        K = int(name)
        sizes = sizes_of(K)
        A, b, w, fold, cls = planted_rows(6000 + K, K, sizes)
    F = len(sizes)
    cat = fold * nsub + (cls if nsub > 1 else 0)
    blocks = blocks_numpy(A, b, w, cat, F * nsub)
    lam = scipy.linalg.eigvalsh(ff.sum_blocks(blocks, nsub)[1][:K * K].reshape(K, K))
    lmax = float(np.max(np.abs(lam)))
    alphas = np.array([f * lmax for f in ALPHA_FRACTIONS])
    # the truncating rcond sits in the middle (geometrically) of the planted gap of the total; 1e-6 where a column repeats
    tail = int(np.count_nonzero(np.arange(K) % 4 == 1))
    if name == "dup":
        rc = 1e-6
    elif tail and tail < K:
        rc = float(np.sqrt(np.sqrt(lam[tail - 1] * lam[tail]) / lmax))
    else:
        rc = 1e-4                                           # no tail to drop (K = 1)
    return A, b, w, fold, cls, blocks, K, F, alphas, np.array([0.0, rc])


def systems(blocks, K, nsub):
    folds, total = ff.sum_blocks(blocks, nsub)
    return folds, total, [ff.downdated(folds, total, f, K) for f in range(folds.shape[0] + 1)]


def cut_of(rcond, n, lmax):
    return max(rcond * rcond, 4.0 * n * EPS) * lmax


def oracle_b(Qm, qv, y2, dead, alphas, rconds):
    """Oracle B of one downdated system: dict with lam (ascending), lmax, and per setting q = ia Qr + ir: kept (mask), beta
    (K, long double sums), rank, dof, sse."""
    K = len(qv)
    live = np.flatnonzero(~dead)
    n = live.size
    out = dict(lam=np.zeros(0), lmax=0.0, n=n, live=live, sets=[])
    if n:
        lam, V = scipy.linalg.eigh(Qm[np.ix_(live, live)])
        out["lam"], out["lmax"] = lam, float(np.max(np.abs(lam)))
        z = V.astype(LD).T @ qv[live].astype(LD)
    for a in alphas:
        for r in rconds:
            beta = np.zeros(K, dtype=LD)
            kept = np.zeros(n, dtype=bool)
            dof, sse = LD(0), LD(y2)
            if n:
                kept = out["lam"] > cut_of(r, n, out["lmax"])
                lk = out["lam"][kept].astype(LD)
                g = z[kept] / (lk + LD(a))
                beta[live] = V[:, kept].astype(LD) @ g
                dof = np.sum(lk / (lk + LD(a)))
                sse = max(LD(y2) - 2 * (g @ z[kept]) + np.sum(lk * g * g), LD(0))
            out["sets"].append(dict(kept=kept, beta=beta, rank=int(kept.sum()), dof=float(dof), sse=float(sse), alpha=float(a),
                                    rcond=float(r)))
    return out


def admit(B, where=""):
    """The admission of one problem's oracle B: asserts the separation from every cut and the planted gap."""
    lam, n = B["lam"], B["n"]
    for st in B["sets"]:
        if not n:
            continue
        cut = cut_of(st["rcond"], n, B["lmax"])
        assert np.all(np.abs(lam / cut - 1.0) >= CUT_MARGIN), (where, st["alpha"], st["rcond"], "an eigenvalue at the cut")
        kept = st["kept"]
        if not kept.all() and kept.any():
            assert lam[kept].min() >= GAP * np.max(np.abs(lam[~kept])), (where, st["rcond"], "planted gap", lam[kept].min(),
                                                                         np.max(np.abs(lam[~kept])))


def oracle_a(Qm, qv, dead, alpha):
    """Oracle A: beta of (Qm + alpha I) beta = qv on the live columns by a long-double Cholesky (K, long double)."""
    live = np.flatnonzero(~dead)
    beta = np.zeros(len(qv), dtype=LD)
    if live.size:
        H = Qm[np.ix_(live, live)].astype(LD) + LD(alpha) * np.eye(live.size, dtype=LD)
        beta[live] = chol_solve_ld(H, qv[live].astype(LD))
    return beta


def rows_sse_ld(A, b, w, rows, beta):
    """Rowwise long-double sum of (w (b - A beta))^2 over ``rows``."""
    r = (np.asarray(b[rows], dtype=LD) - np.asarray(A[rows], dtype=LD) @ np.asarray(beta, dtype=LD)) * np.asarray(w[rows], dtype=LD)
    return float(r @ r)


def scaled_err(Qm, beta, ref):
    """max |d (beta - ref)| / max |d ref|, d = sqrt(diag Qm) (the difference itself when the reference vanishes)."""
    d = np.sqrt(np.maximum(np.diag(Qm), 0.0)).astype(LD)
    num = float(np.max(np.abs(d * (np.asarray(beta, dtype=LD) - ref)))) if len(ref) else 0.0
    den = float(np.max(np.abs(d * ref))) if len(ref) else 0.0
    return num / den if den > 0 else num


def unit_of(B, st):
    """The error unit of a setting: n_live eps lambda_max / (smallest kept lambda + alpha) (n_live eps with nothing kept)."""
    n = max(B["n"], 1)
    if not st["kept"].any():
        return n * EPS
    return n * EPS * B["lmax"] / (float(B["lam"][st["kept"]].min()) + st["alpha"])


def held_scale(block, K, beta):
    G, c, bb, _ = ff.unpack(block, K)
    ab = np.abs(np.asarray(beta, dtype=np.float64))
    return bb + 2.0 * float(ab @ np.abs(c)) + float(ab @ (np.abs(G) @ ab))


def figures(name, nsub, out, coef_bar=None, where=""):
    """The worst ratios of ``out`` = (eig, z, info, sets, fits, coef, heldout) -- a route's result on case ``name`` -- against
    the oracles, after admitting every problem and asserting equal ranks, n_live and supports: dict(coef, eig, scalar, held).
    No truncation active (every direction kept): oracle A and the rowwise sse; otherwise oracle B."""
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = case(name, nsub)
    eig, z, info, sets, fits, coef, held = out
    folds, total, sys_ = systems(blocks, K, nsub)
    Qr = len(rconds)
    worst = dict(coef=0.0, eig=0.0, scalar=0.0, held=0.0)
    if name not in VARIANTS:
        worst["eig_rel"] = 0.0
    for f in range(F + 1):
        Qm, qv, y2, _, dead = sys_[f]
        B = oracle_b(Qm, qv, y2, dead, alphas, rconds)
        at = (where, name, nsub, f)
        admit(B, at)
        n = B["n"]
        assert info[f, 0] == n and info[f, 5] == 0, (at, info[f])
        assert not eig[f, n:].any() and not z[f, n:].any(), at
        if n:
            worst["eig"] = max(worst["eig"], float(np.max(np.abs(eig[f, :n] - B["lam"]))) / (n * EPS * B["lmax"]))
        # the sweep cases are well scaled (asserted): every eigenvalue relative to ITSELF, against long-double Jacobi -- every
        # problem with the folds alone, the fit on all rows with fold x class blocks (the reference takes a second at K = 144)
        if n and name not in VARIANTS and (nsub == 1 or f == F):
            ref = eig_ld(well_scaled(Qm, B["live"]))
            worst["eig_rel"] = max(worst["eig_rel"], float(np.max(np.abs(eig[f, :n].astype(LD) / ref - 1))) / (n * EPS))
        train = fold != f
        for q, st in enumerate(B["sets"]):
            beta = fits[q] if f == F else coef[f, q]
            assert sets[f, q, 0] == st["rank"], (at, q, sets[f, q, 0], st["rank"])
            assert not np.any(beta[dead]), (at, q)
            unit = unit_of(B, st)
            full = n > 0 and st["rank"] == n
            ref = oracle_a(Qm, qv, dead, st["alpha"]) if full else st["beta"]
            worst["coef"] = max(worst["coef"], scaled_err(Qm, beta, ref) / unit)
            sse_ref = rows_sse_ld(A, b, w, np.flatnonzero(train), ref) if full else st["sse"]
            fig = max(abs(sets[f, q, 1] - st["dof"]) / max(n, 1), abs(sets[f, q, 2] - sse_ref) / y2 if y2 > 0 else 0.0)
            worst["scalar"] = max(worst["scalar"], fig / unit)
            if f < F:
                for s in range(nsub):
                    rows = np.flatnonzero((fold == f) & ((cls == s) if nsub > 1 else True))
                    blk = blocks[f * nsub + s]
                    assert held[f, q, s, 0] == len(rows) and held[f, q, s, 2] == blk[K * K + K], (at, q, s)
                    true = rows_sse_ld(A, b, w, rows, beta)
                    scale = held_scale(blk, K, beta)
                    if scale > 0:
                        worst["held"] = max(worst["held"], abs(held[f, q, s, 1] - true) / (EPS * scale))
                    else:
                        assert held[f, q, s, 1] == 0.0, (at, q, s)
    return worst


def against_host(name, nsub, dev, host, where=""):
    """``against_host_blocks`` on case ``name``; the sweep cases are well scaled, so their eigenvalues are also compared
    relative to each eigenvalue (``eig_rel``, in units of n_live eps)."""
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = case(name, nsub)
    worst = against_host_blocks(blocks, K, nsub, alphas, rconds, dev, host, (where, name))
    if name not in VARIANTS:
        worst["eig_rel"] = 0.0
        for f in range(F + 1):
            n = int(host[2][f, 0])
            if n:
                worst["eig_rel"] = max(worst["eig_rel"], float(np.max(np.abs(dev[0][f, :n] / host[0][f, :n] - 1.0))) / (n * EPS))
    return worst


def against_host_blocks(blocks, K, nsub, alphas, rconds, dev, host, where=""):
    """The kernel's result against the host route's on the same blocks: equal n_live, status and ranks (asserted), and the
    worst differences in the units of ``figures`` (the held-out sums are checked against the rows, in ``figures``; here their
    counts and bb are equal)."""
    folds, total, sys_ = systems(blocks, K, nsub)
    F = folds.shape[0]
    worst = dict(coef=0.0, eig=0.0, scalar=0.0)
    assert np.array_equal(dev[2][:, [0, 5]], host[2][:, [0, 5]]), where
    assert np.array_equal(dev[3][:, :, 0], host[3][:, :, 0]), where
    assert np.array_equal(dev[6][..., [0, 2]], host[6][..., [0, 2]]), where
    for f in range(F + 1):
        Qm, qv, y2, _, dead = sys_[f]
        B = oracle_b(Qm, qv, y2, dead, alphas, rconds)
        n = B["n"]
        if n:
            worst["eig"] = max(worst["eig"], float(np.max(np.abs(dev[0][f] - host[0][f]))) / (n * EPS * B["lmax"]))
        for q, st in enumerate(B["sets"]):
            unit = unit_of(B, st)
            bd, bh = (dev[4][q], host[4][q]) if f == F else (dev[5][f, q], host[5][f, q])
            worst["coef"] = max(worst["coef"], scaled_err(Qm, bd, bh.astype(LD)) / unit)
            fig = max(abs(dev[3][f, q, 1] - host[3][f, q, 1]) / max(n, 1), abs(dev[3][f, q, 2] - host[3][f, q, 2]) / y2 if y2 > 0 else 0.0)
            worst["scalar"] = max(worst["scalar"], fig / unit)
    return worst


def check_bars(worst, factor, where="", name=None):
    bars = dict(coef=MEASURED_COEF_DUP if name == "dup" else MEASURED_COEF, eig=MEASURED_EIG, scalar=MEASURED_SCALAR,
                held=MEASURED_HELD, eig_rel=MEASURED_EIG_REL)
    for key, v in worst.items():
        assert v <= factor * bars[key], (where, key, v, factor * bars[key])


def eig_mp(M):
    """The eigenvalues of the float64 symmetric matrix M by mpmath at 50 digits, ascending, as float64."""
    import mpmath

    with mpmath.workdps(50):
        E = mpmath.eigsy(mpmath.matrix(M.tolist()), eigvals_only=True)
        return np.sort(np.array([float(x) for x in E]))


def eig_ld(M, vectors=False):
    """The eigenvalues (ascending, long double) of the symmetric matrix M by two-sided Jacobi rotations carried in long double,
    the disjoint pairs of a round-robin round rotated at once; with ``vectors`` also the eigenvectors as rows.  On a matrix
    whose diagonally scaled form is well conditioned every eigenvalue is accurate to about n x 1e-19 RELATIVE (Demmel-Veselic),
    which makes this the reference of the relative eigenvalue bars where mpmath (``eig_mp``) would take minutes; the CPU tests
    hold it to ``eig_mp`` at K = 17 and 31."""
    T = np.array(M, dtype=LD)
    n = T.shape[0]
    V = np.eye(n, dtype=LD)
    m = n + (n & 1)
    rounds = []
    for r in range(m - 1):
        a = np.array([m - 1] + [(r + k) % (m - 1) for k in range(1, m // 2)])
        b = np.array([r] + [(r - k) % (m - 1) for k in range(1, m // 2)])
        P, Q = np.minimum(a, b), np.maximum(a, b)
        rounds.append((P[Q < n], Q[Q < n]))
    extra = 0
    for _ in range(80):
        off = float(np.sum(np.tril(T, -1) ** 2))
        if off == 0.0 or off <= 1e-34 * float(np.sum(np.diag(T) ** 2)):
            extra += 1                                      # two more sweeps: down to the rounding of long double
            if off == 0.0 or extra > 2:
                break
        for P, Q in rounds:
            if not P.size:
                continue
            app, aqq, apq = T[P, P], T[Q, Q], T[P, Q]
            nz = apq != 0
            theta = np.zeros_like(apq)
            theta[nz] = (aqq[nz] - app[nz]) / (2 * apq[nz])
            t = np.where(nz, np.where(theta >= 0, LD(1), LD(-1)) / (np.abs(theta) + np.sqrt(theta * theta + 1)), LD(0))
            c = 1 / np.sqrt(t * t + 1)
            sn = t * c
            Tp, Tq = T[P, :].copy(), T[Q, :].copy()
            T[P, :], T[Q, :] = c[:, None] * Tp - sn[:, None] * Tq, sn[:, None] * Tp + c[:, None] * Tq
            Tp, Tq = T[:, P].copy(), T[:, Q].copy()
            T[:, P], T[:, Q] = c[None, :] * Tp - sn[None, :] * Tq, sn[None, :] * Tp + c[None, :] * Tq
            T[P, Q] = T[Q, P] = 0
            T[P, P], T[Q, Q] = app - t * apq, aqq + t * apq
            if vectors:
                Vp, Vq = V[P, :].copy(), V[Q, :].copy()
                V[P, :], V[Q, :] = c[:, None] * Vp - sn[:, None] * Vq, sn[:, None] * Vp + c[:, None] * Vq
    lam = np.diag(T).copy()
    order = np.argsort(lam, kind="stable")
    return (lam[order], V[order]) if vectors else lam[order]


def well_scaled(Qm, live):
    """The live block of Qm, after asserting that its diagonally scaled form has a condition number <= 1e3."""
    H = Qm[np.ix_(live, live)]
    d = 1.0 / np.sqrt(np.diag(H))
    assert np.linalg.cond(H * np.outer(d, d)) <= 1e3
    return H


def host_route(name, nsub=1):
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = case(name, nsub)
    return sp.spectral_path_host(blocks, K, alphas, rconds, nsub)


ALL_CASES = [(K, ns) for K in SWEEP_K + LDS_EDGE_K for ns in (1, 3)] + [(v, 1) for v in VARIANTS]


def measure(path=None):
    """Measures the host route against the oracles over ALL_CASES and writes the record."""
    lines = ["# host route (fsnap_spectral_gram per problem) against oracles A / B; written by tests/spectral_path_cases.py",
             "# ratios: see MEASURED_* in tests/spectral_path_cases.py", "case nsub    coef     eig      eig_rel  scalar   held   sweeps"]
    worst = dict(coef=0.0, eig=0.0, scalar=0.0, held=0.0, eig_rel=0.0)
    dup = 0.0
    for name, ns in ALL_CASES:
        out = host_route(name, ns)
        fig = figures(name, ns, out, where="measure")
        fig.setdefault("eig_rel", 0.0)
        lines.append(f"{str(name):>5} {ns}   {fig['coef']:.2e} {fig['eig']:.2e} {fig['eig_rel']:.2e} {fig['scalar']:.2e} "
                     f"{fig['held']:.2e}  {int(out[2][:, 1].min())}...{int(out[2][:, 1].max())}")
        print(lines[-1], flush=True)
        if name == "dup":
            dup, fig["coef"] = fig["coef"], 0.0
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    mp = 0.0
    for K in (17, 31):                                      # the long-double reference itself against mpmath at 50 digits
        A, b, w, fold, cls, blocks, _, F, alphas, rconds = case(K)
        H = well_scaled(systems(blocks, K, 1)[2][F][0], np.arange(K))
        mp = max(mp, float(np.max(np.abs(eig_ld(H) / eig_mp(H) - 1))) / (K * EPS))

    def up(v):                                              # two digits, rounded UP: a constant is never below its record
        return float(f"{v:.1e}") if float(f"{v:.1e}") >= v else float(f"{v * 1.05:.1e}")

    lines.append(f"MEASURED_COEF = {up(worst['coef']):.1e}  MEASURED_COEF_DUP = {up(dup):.1e}  MEASURED_EIG = {up(worst['eig']):.1e}  "
                 f"MEASURED_EIG_REL = {up(worst['eig_rel']):.1e}  MEASURED_SCALAR = {up(worst['scalar']):.1e}  "
                 f"MEASURED_HELD = {up(worst['held']):.1e}   (rounded up; eig_ld against mpmath: {mp:.1e} n eps)")
    print(lines[-1])
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    measure(os.path.join(ROOT, "profiles", "spectral_path_accuracy.txt"))
