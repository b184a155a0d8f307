"""Cases, references and bars of the BCS solver and its grouped K-fold paths (tests/test_bcs_cpu.py,
tests/test_gpu_bcs_path.py).

Goldens: tests/golden/bcs_reference.npz holds what the reference's own ``bcs()`` returns on the Ta rows (all, with a testing
mask, through the transpose substitution) and on small synthetic systems, two of which make it go through a deletion
(tests/golden/make_golden_bcs.py).  ``case_statistics`` forms (A^T A, A^T y, |y|^2, sum y, n) of a case in ``numpy.longdouble``
and rounds once: the bars of the issue are about the recurrence on the statistics, and a float64 ``aw.T @ aw`` of the Ta rows
(condition number 7e10) alone moves the clipped Sig by 2e-8 of its largest entry, four times what the recurrence does.

Direct posterior: for a run whose state is consistent (``deletion="exact"``, or no deletion) the returned (active, alpha,
sigma2_in) determine Sigma = (diag alpha + Q_ss / sigma2)^-1 and mu = Sigma q_s / sigma2; ``posterior_ld`` solves that in long
double.

Path cases (``PATH_CASES``): rows of O(1) columns in ``NCONF`` configurations with three row classes, a sparse truth plus
noise; ``case_blocks`` packs them per (fold, class) in long double.  Picks are discrete, so a case is used for the comparison of
picks only if the host route's ``margin`` -- the smallest relative gap between the best and the second-best marginal likelihood
over a problem's iterations -- is at least ``MIN_MARGIN`` in every problem; the CPU test asserts it for every case listed here.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import bcs_path as bp  # noqa: E402
from fitsnap_amd.solvers import folds as ff  # noqa: E402

LD = np.longdouble
GOLDEN = os.path.join(ROOT, "tests", "golden")
MIN_MARGIN = 1e-3                 # the issue's: every case used for pick comparison
REF_BAR = 1e-8                    # the issue's: host route against the reference, relative to the largest entry
POSTERIOR_BAR = 1e-10             # the issue's: "exact" runs against the direct posterior on well-conditioned cases
# Device against the host route on the same statistics, relative to the largest entry of each output.  The issue sets the bar
# at 100 x the largest difference measured on the MI355X over PATH_CASES, never looser than REF_BAR: measured 6.071e-13 (case
# k128, in a held-out sum; profiles/bcs_path_timing.txt), so 6.071e-11.
DEVICE_MEASURED = 6.071e-13
DEVICE_BAR = min(100 * DEVICE_MEASURED, REF_BAR)
NCONF, NCLASS = 40, 3


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "bcs_reference.npz"))
    return {k: z[k] for k in z.files}


def tags():
    return [str(t) for t in golden()["tags"]]


def synthetic(m, K, c, nnz, noise, seed):
    """The synthetic rows of tests/golden/make_golden_bcs.py (restated here so that the goldens can be checked for drift)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, K))
    A = X @ (np.eye(K) + c * rng.standard_normal((K, K)) / np.sqrt(K))
    truth = np.zeros(K)
    sup = rng.choice(K, size=min(nnz, K), replace=False)
    truth[sup] = rng.standard_normal(len(sup)) * 2.0
    y = A @ truth + noise * rng.standard_normal(m)
    return A, y


def case_rows(tag, ta):
    """(aw, bw) of a golden case: the weighted rows the reference's bcs() was given."""
    g = golden()
    if tag.startswith("ta"):
        A, b, w = ta
        keep = ~g[f"{tag}_testing"]
        aw, bw = (w[:, None] * A)[keep], (w * b)[keep]
        if tag == "ta_transpose":
            return aw.T @ aw, aw.T @ bw                # float64, as the reference forms its "rows"
        return aw, bw
    return g[f"{tag}_A"], g[f"{tag}_y"]


def statistics_ld(aw, bw):
    """(Q, q, y2, sum_y, n) in long double, rounded once."""
    L, y = np.asarray(aw, dtype=LD), np.asarray(bw, dtype=LD)
    return (np.ascontiguousarray((L.T @ L).astype(np.float64)), np.ascontiguousarray((L.T @ y).astype(np.float64)), float(y @ y),
            float(y.sum()), float(len(y)))


def case_statistics(tag, ta):
    return statistics_ld(*case_rows(tag, ta))


def expected(tag):
    g = golden()
    return {k: g[f"{tag}_{k}"] for k in ("weights", "errbars", "used", "sigma2", "Sig", "deletions")}


def rel(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref))) if ref.size else 0.0


def posterior_ld(Q, q, active, alpha, sigma2):
    """(mu, Sigma) of the direct posterior on the support, in long double."""
    s = np.asarray(active, dtype=np.int64)
    H = np.diag(np.asarray(alpha, dtype=LD)) + np.asarray(Q, dtype=LD)[np.ix_(s, s)] / LD(sigma2)
    n = len(s)
    # Gauss-Jordan in long double (numpy.linalg has no long double)
    M = np.concatenate([H, np.eye(n, dtype=LD)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    Sigma = M[:, n:]
    mu = Sigma @ (np.asarray(q, dtype=LD)[s] / LD(sigma2))
    return mu, Sigma


# ---- rows and blocks of the path cases ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rows(seed, K, per=25, nnz=None, noise=0.3, nconf=NCONF, mix=1.0):
    """(A, b, w, configuration per row, class per row): O(1) Gaussian columns mixed by I + mix N / sqrt(K), a sparse truth of ``nnz``
    entries (default: about a sixth of the columns, at least one) plus noise, weights in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    m = nconf * per
    A = rng.standard_normal((m, K)) @ (np.eye(K) + mix * rng.standard_normal((K, K)) / np.sqrt(K))
    nnz = max(1, K // 6) if nnz is None else min(nnz, K)
    truth = np.zeros(K)
    sup = rng.choice(K, size=nnz, replace=False)
    truth[sup] = rng.standard_normal(nnz) * 2.0 + np.sign(rng.standard_normal(nnz))
    b = A @ truth + noise * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    conf = np.repeat(np.arange(nconf), per).astype(np.int64)
    cls = (np.arange(m) % NCLASS).astype(np.int64)
    for x in (A, b, w, conf, cls):
        x.setflags(write=False)
    return A, b, w, conf, cls


def blocks_ld(A, b, w, cat, ncat):
    """The packed per-category blocks [G | c | bb, sum wb, n] formed in long double and rounded once: ncat x (K^2 + K + 3).
    cat < 0: the row takes no part."""
    K = A.shape[1]
    out = np.zeros((ncat, K * K + K + 3))
    for c in range(ncat):
        r = np.flatnonzero(cat == c)
        X = np.asarray(A[r], dtype=LD) * np.asarray(w[r], dtype=LD)[:, None]
        y = np.asarray(b[r], dtype=LD) * np.asarray(w[r], dtype=LD)
        out[c, :K * K] = (X.T @ X).ravel().astype(np.float64)
        out[c, K * K:K * K + K] = (X.T @ y).astype(np.float64)
        out[c, K * K + K:] = (float(y @ y), float(y.sum()), len(r))
    return out


# name: (seed, K, F (None: every configuration its own fold), nsub, grid, max_active, deletion, rows keywords)
# K on the boundaries of the column ownership (lanes and waves); the grids cover itermax 1 / 10 / 80, sigma2 given and from
# scale, Q = 1 and 3; max_active 1, 2 and 64 ("fill": 64 columns enter and the full set blocks every further addition).
G1 = ({"scale": 0.01, "itermax": 10},)
G3 = ({"scale": 0.01, "itermax": 1}, {"scale": 1e-3, "itermax": 10}, {"sigma2": 0.05, "itermax": 80, "eta": 1e-8})
GD = ({"scale": 0.01, "itermax": 60}, {"scale": 1e-3, "itermax": 60}, {"scale": 0.1, "itermax": 60})
# "del_ref" / "del_exact": 200 rows of strongly correlated columns (mix = 3) with noise 0.5, on which the recurrence goes through
# many deletions (host route: 17 / 21 over the 18 problems) -- the compaction of Sig, the shift of the active rows and, in exact
# mode, the updates of mu, S and Q; DELETION_CASES names them and the number of BCS_DEL picks every one must at least show.
DELETION_CASES = {"del_ref": 10, "del_exact": 10}
PATH_CASES = {
    "k1": (1, 1, 2, 1, G3, 1, "reference", {}),
    "k2": (2, 2, 5, 3, G3, 2, "exact", {}),
    "k63": (63, 63, 2, 3, G3, 63, "reference", {}),
    "k64": (64, 64, 5, 1, G3, 64, "exact", {}),
    "k65": (65, 65, 2, 1, G1, 64, "reference", {}),
    "k128": (1005, 128, 5, 3, G3, 64, "reference", {}),
    "k129": (129, 129, 2, 1, G3, 2, "exact", {}),
    "k144": (2020, 144, 5, 1, G3, 64, "exact", {}),
    "k144_one": (145, 144, 2, 3, G1, 1, "reference", {}),
    "loco": (33, 33, None, 1, G1, 33, "reference", {}),
    "del_ref": (5030, 33, 5, 1, GD, 33, "reference", {"mix": 3.0, "nnz": 6, "noise": 0.5, "per": 5}),
    "del_exact": (5030, 33, 5, 1, GD, 33, "exact", {"mix": 3.0, "nnz": 6, "noise": 0.5, "per": 5}),
    "fill": (3010, 144, 2, 1, ({"scale": 1e-5, "itermax": 80},), 64, "reference", {"nnz": 100, "noise": 0.05}),
}


def case_settings(name):
    seed, K, F, nsub, grid, max_active, deletion, kw = PATH_CASES[name]
    section = type("S", (), dict(sigma2=None, scale=0.01, eta=1e-18, itermax=10))
    return seed, K, NCONF if F is None else F, nsub, bp.resolve_grid(grid, section), max_active, deletion, kw


@functools.lru_cache(maxsize=None)
def case_blocks(name):
    """(blocks (F * nsub x (K^2 + K + 3)), K, F, nsub, hyper (Q x 4), max_active, deletion) of a path case."""
    seed, K, F, nsub, grid, max_active, deletion, kw = case_settings(name)
    A, b, w, conf, cls = rows(seed, K, **kw)
    fold = conf % F
    cat = fold * nsub + (cls if nsub > 1 else 0)
    blocks = blocks_ld(A, b, w, cat, F * nsub)
    blocks.setflags(write=False)
    return blocks, K, F, nsub, bp.hyper_of(grid), max_active, deletion


@functools.lru_cache(maxsize=None)
def case_host(name):
    """The host route's (coef, active, alpha, errbars, picks, info, heldout, Sig) of a path case: computed once, shared."""
    blocks, K, F, nsub, hyper, max_active, deletion = case_blocks(name)
    out = bp.bcs_path_host(blocks, K, hyper, max_active, deletion, nsub)
    for x in out:
        x.setflags(write=False)
    return out


def edge_blocks(F=3):
    """K = 12 rows in F folds: column 3 is zero and fold 1 alone touches column 7.  (blocks, K)"""
    K = 12
    A, b, w, conf, _ = rows(7, K, nnz=4)
    A, b = A.copy(), b.copy()
    fold = conf % F
    A[:, 3] = 0.0
    A[fold != 1, 7] = 0.0
    b = b + 2.0 * A[:, 7]
    return blocks_ld(A, b, w, fold, F), K


def downdated_scalars(blocks, nsub, f, K):
    """(Qm, qv, y2, sum_y, n, tdiag) of problem f as both routes form them."""
    folds, total = ff.sum_blocks(blocks, nsub)
    Qm, qv, y2, n, _ = ff.downdated(folds, total, f, K)
    at = K * K + K
    sum_y = total[at + 1] - folds[f, at + 1] if f < folds.shape[0] else total[at + 1]
    return Qm, qv, y2, float(sum_y), n, np.ascontiguousarray(np.diag(ff.unpack(total, K)[0]))
