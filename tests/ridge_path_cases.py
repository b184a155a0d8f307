"""Helpers shared by tests/test_ridge_path_cpu.py, tests/test_gpu_ridge_path.py and tests/ridge_path_dist_worker.py: the
long-double refit of one unit over a grid of alphas with the intermediates the a-priori bar needs (``unit_ld``), the bar
(``kernel_bar``), the errors of a sweep cell (``measure``) and the interior-minimum case (``interior_case``).  The rows,
units and the long-double linear algebra are those of tests/loco_cases.py, imported, not copied."""
import numpy as np

import loco_cases as lc
from fitsnap_amd.solvers import ridge_path as rp

LD = lc.LD
EPS = lc.EPS
SWEEP_K = [1, 2, 15, 16, 17, 31, 33, 64, 110, 128, 129, 142, 144]
ALPHAS = [0.0, 1e-8, 1e-4, 1.0, 1e2]
NCLASS = 3


def row_classes(m):
    return (np.arange(m) % NCLASS).astype(np.uint8)


def unit_ld(A, b, w_eff, stats, rows, alphas, precise=True):
    """The refit without the rows ``rows`` at every alpha, in long double (``precise``; float64 otherwise, enough for a bar)
    on the long-double statistics ``stats`` = (G, c): list over the alphas of dicts "pred" (float64), "beta", "d" (diag B_q),
    "kappa" (kappa_2 of H_q = D^-1 B_q D^-1), "rho" (max_j (G_jj + alpha) / (G_jj - G_u,jj + alpha)), "minpiv" (smallest
    Cholesky pivot of H_q) and "ok" (B_q has a positive diagonal and H_q is positive definite); a dict with ok False has
    nothing else."""
    T = LD if precise else np.float64
    Ac = np.asarray(A)[rows].astype(T)
    w = np.asarray(w_eff)[rows].astype(T)
    X = Ac * w[:, None]
    G, c = (np.asarray(s).astype(T) for s in stats)
    K = G.shape[0]
    base = G - X.T @ X
    rhs = c - X.T @ (w * np.asarray(b)[rows].astype(T))
    out = []
    for alpha in alphas:
        B = base + T(alpha) * np.eye(K, dtype=T)
        d = np.diag(B).copy()
        if not np.all(d > 0):
            out.append({"ok": False})
            continue
        s = np.sqrt(d)
        H = B / s[:, None] / s[None, :]
        if precise:
            L, piv, ok = lc.cholesky_ld(H)
        else:
            try:
                piv, ok = np.diag(np.linalg.cholesky(H)) ** 2, True
            except np.linalg.LinAlgError:
                piv, ok = np.zeros(1), False
        if not ok:
            out.append({"ok": False})
            continue
        x = lc.solve_ld(H, rhs / s) if precise else np.linalg.solve(H, rhs / s)
        beta = x / s
        out.append({"ok": True, "pred": (Ac @ beta).astype(np.float64), "beta": beta.astype(np.float64),
                    "d": d.astype(np.float64), "kappa": float(np.linalg.cond(H.astype(np.float64))),
                    "rho": float(np.max((np.diag(G) + T(alpha)) / d)), "minpiv": float(np.min(piv))})
    return out


def kernel_bar(Ac, ref):
    """A-priori rounding bar of the refit predictions p_i = a_i . beta of one unit's rows ``Ac`` at one alpha, per row:

        4 eps [ K (|a_i| . |beta|) + (2 K + n_u) rho_u kappa_2(H_q) ||a_i D_q^-1|| ||D_q beta|| ]

    from the inputs and the REFERENCE's intermediates only (``ref``: one dict of ``unit_ld``; beta, D_q = sqrt(diag B_q),
    kappa_2(H_q) and rho_u = max_j (G_jj + alpha) / (G_jj - G_u,jj + alpha) are the long-double refit's, never the kernel's).

    Derivation, with gamma_k ~ k eps the bound of a serial FMA chain of length k.  The kernel returns a_i . beta^ with the
    computed beta^: the product is a chain of length K over the k index (the MFMA accumulates it in order), error
    <= gamma_K |a_i| . |beta^|: the first term.  The second is |a_i . (beta^ - beta)| = |(a_i D^-1) . D (beta^ - beta)|
    <= ||a_i D^-1|| ||D (beta^ - beta)||, and z = D beta solves H z = D^-1 r with H = D^-1 B D^-1 of unit diagonal.  What the
    kernel solves differs from that system by (a) the rounding of G_u: every entry is a chain of n_u products,
    |dG_u| <= gamma_{n_u} |X_u|^T |X_u|, whose entries are bounded by sqrt(G_u,ii G_u,jj) <= sqrt((G_ii + alpha)(G_jj + alpha))
    <= rho_u sqrt(B_ii B_jj): after the scaling an entrywise perturbation of H of at most gamma_{n_u} rho_u, likewise
    gamma_{n_u} rho_u for the scaled right-hand side (c_u is the same chain); the subtraction G - G_u and the two scalings add
    3 roundings of entries that are <= rho_u in the scaled units; (b) the Cholesky factorisation and the two triangular solves
    of order K, backward stable with gamma_{K + 1} + 2 gamma_K |L| |L^T| <= ~2 K eps entrywise on a matrix of unit diagonal.
    A perturbation dH changes z by ||dz|| <= kappa_2(H) ||dH|| ||z|| / ||H|| to first order, with ||H|| >= 1 (unit diagonal).
    Counting the entrywise bounds above as the norm of dH (they are entries of positive semi-definite matrices with diagonal
    <= rho_u, whose norm is between rho_u and K rho_u: rho_u is exact for uncorrelated columns and optimistic by the
    largest eigenvalue of the columns' correlation matrix otherwise -- the factor 4, and kappa_2 being attained by one
    direction only, carry that) gives (n_u + 2 K) eps rho_u kappa_2(H_q) ||D beta||, the second term.  The constant 4 is that
    of loco_cases.kernel_bar (two roundings per FMA step counted separately, and a factor 2 of slack).

    Measured on an MI355X by tests/test_gpu_ridge_path.py's sweep (every cell prints its line; all of them are in
    profiles/ridge_path_accuracy.txt).  Per K, worst over alpha = 0, 1e-8, 1e-4, 1, 1e2: worst row error / bar, then the
    kernel's RMS error over ridge_path_host's, both against the long-double refit:

    K =   1: 0.1 / 1.75
    K =   2: 0.15 / 0.968
    K =  15: 0.011 / 1.06
    K =  16: 0.013 / 1.02
    K =  17: 0.0075 / 1.07
    K =  31: 0.0027 / 1.11
    K =  33: 0.0041 / 1.11
    K =  64: 0.0011 / 1.14
    K = 110: 0.00045 / 1.26
    K = 128: 0.00044 / 1.24
    K = 129: 0.00032 / 1.26
    K = 142: 0.00032 / 1.19
    K = 144: 0.0004 / 1.17

    Worst error / bar 0.15 (K = 2, where the bar is a few eps wide); worst RMS ratio 1.75 (K = 1, both errors ~1e-16).  On
    the CPU, ridge_path_host itself: 0.0056 (K = 17), 0.00031 (K = 144).  The Woodbury route and Solver.loco_errors against
    the kernel, over the sum of this bar and loco_cases.kernel_bar: 0.001.
    """
    aa = np.abs(np.asarray(Ac, dtype=np.float64))
    n, K = aa.shape
    beta = np.asarray(ref["beta"], dtype=np.float64)
    s = np.sqrt(np.asarray(ref["d"], dtype=np.float64))
    return 4 * EPS * (K * (aa @ np.abs(beta))
                      + (2 * K + n) * ref["rho"] * ref["kappa"] * np.linalg.norm(aa / s[None, :], axis=1) * np.linalg.norm(s * beta))


def measure(A, b, w_eff, stats, rows, off, alphas, preds, host_preds, ld_units=None):
    """Errors of the Q x m predictions ``preds`` of one K: units with ld_units[u] (default: all) against the long-double
    refit, the others against ``host_preds`` (ridge_path_host), every row against the bar of its unit and alpha.  dict of
    (Q x nunits) arrays "ratio" (worst row error / bar; inf where the reference is not positive definite or a prediction is
    not finite), "minpiv", "kappa", "rho" and the per-alpha vectors "rms_pred", "rms_host" over the long-double rows."""
    Q, nunits = len(alphas), len(off) - 1
    out = {k: np.zeros((Q, nunits)) for k in ("ratio", "minpiv", "kappa", "rho")}
    se_pred, se_host, nld = np.zeros(Q), np.zeros(Q), 0
    for u in range(nunits):
        r = np.asarray(rows[off[u]:off[u + 1]])
        ld = ld_units is None or bool(ld_units[u])
        refs = unit_ld(A, b, w_eff, stats, r, alphas, precise=ld)
        nld += len(r) if ld else 0
        for q, ref in enumerate(refs):
            if not ref["ok"]:
                out["ratio"][q, u] = np.inf
                continue
            truth = ref["pred"] if ld else host_preds[q, r]
            err = np.abs(preds[q, r] - truth)
            err[~np.isfinite(err)] = np.inf
            out["ratio"][q, u] = np.max(err / kernel_bar(A[r], ref))
            for k in ("minpiv", "kappa", "rho"):
                out[k][q, u] = ref[k]
            if ld:
                se_pred[q] += float(np.sum((preds[q, r] - truth) ** 2))
                se_host[q] += float(np.sum((host_preds[q, r] - truth) ** 2))
    out["rms_pred"] = np.sqrt(se_pred / max(nld, 1))
    out["rms_host"] = np.sqrt(se_host / max(nld, 1))
    return out


def cell_line(K, alpha, res, q):
    rr = res["rms_pred"][q] / res["rms_host"][q] if res["rms_host"][q] > 0 else np.inf
    return (f"PATH K={K} alpha={alpha:g}: worst err/bar {np.max(res['ratio'][q]):.3g}  rms/host {rr:.3g}  "
            f"(rms {res['rms_pred'][q]:.3g}, host {res['rms_host'][q]:.3g})  min pivot {np.min(res['minpiv'][q]):.3g}  "
            f"kappa {np.max(res['kappa'][q]):.3g}  rho {np.max(res['rho'][q]):.3g}")


def own_sums(b, w_eff, preds_q, rows, row_class, nclass):
    """((nclass x 4) sums of one unit at one alpha from the given predictions, summed in long double with the kernel's
    per-term roundings (r = b - p and w r rounded to float64), and the (nclass x 4) sums of the terms' magnitudes)."""
    r = b[rows] - preds_q[rows]
    wr = w_eff[rows] * r
    terms = np.stack([np.ones(len(rows), dtype=LD), np.abs(r).astype(LD), r.astype(LD) ** 2, wr.astype(LD) ** 2], axis=1)
    cls = row_class[rows]
    out = np.zeros((nclass, 4), dtype=LD)
    for k in range(nclass):
        out[k] = terms[cls == k].sum(axis=0)
    return out


def interior_case():
    """default_rng(5), K = 33, 12 units of 5 rows, A standard normal, b = A beta + 2 standard normal, w uniform(0.5, 2),
    alphas = logspace(-6, 3, 10): the total weighted LOO SSE has its minimum at alpha = 10 (1049.47 at 1e-6, 972.29 at 10,
    1777.9 at 1e2).  Returns (A, b, w, labels, alphas)."""
    rng = np.random.default_rng(5)
    K, nu, n = 33, 12, 5
    m = nu * n
    A = rng.standard_normal((m, K))
    b = A @ rng.standard_normal(K) + 2.0 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    cfg = np.repeat(np.arange(nu), n)
    labels = {"Configs": [f"cfg{c}" for c in cfg], "Groups": [f"g{c % 3}" for c in cfg], "Testing": [False] * m,
              "Row_Type": [("Energy", "Force", "Stress")[i % 3] for i in range(m)]}
    return A, b, w, labels, np.logspace(-6, 3, 10)


def host_path(A, b, w_eff, alphas, labels, by="Configs"):
    """ridge_path_host of labelled rows: (sums, info, preds, sorted_rows, offsets, units, class names, row classes)."""
    train = ~np.asarray(labels.get("Testing", [False] * len(b)), dtype=bool)
    w_eff = np.where(train, w_eff, 0.0)
    Aw = A * w_eff[:, None]
    rows, off, units = rp.loco.unit_index(labels[by], train)
    names = sorted(set(labels["Row_Type"]))
    cls = np.array([names.index(t) for t in labels["Row_Type"]], dtype=np.uint8)
    sums, info, preds = rp.ridge_path_host(A, b, w_eff, Aw.T @ Aw, Aw.T @ (b * w_eff), alphas, rows, off, cls, len(names))
    return sums, info, preds, rows, off, units, names, cls
