"""Cases, yardstick and error bars of the greedy sparse-selection paths (tests/test_omp_path_cpu.py,
tests/test_gpu_omp_path.py).

Rows: about 1 500 in 60 configurations of 25, three row classes, columns scaled over six decades, a sparse truth plus noise.
The packed per-category blocks are formed in long double and rounded once (``blocks_ld``), or come from the GPU.

Yardstick: ``omp_ld`` -- the recurrence of ``fsnap_omp_gram`` (include/fsnap_hip.h) restated in ``numpy.longdouble`` on the
float64 downdated system the code under test sees.  It also returns, per step, the relative margin between the best and the
second-best score: selection is discrete, so every committed case must keep a margin >= ``MIN_MARGIN`` (the CPU test asserts
it for every case and problem; no comparison is skipped or softened).

Independent checks: scikit-learn's ``orthogonal_mp_gram`` on the column-normalised Gram matrix ("omp") and brute-force forward
stepwise regression on the rows ("ols": the column whose least-squares refit leaves the smallest residual).

Error bars (``bars``): with beta_ld the yardstick's coefficients after s steps -- the long-double solve on that support --
  coefficients   max |beta - beta_ld| <= max(16 err64, 64 eps max |beta_ld|),  err64 = max |numpy.linalg.solve(Qm_SS, qv_S) - beta_ld|
  e_s            |e - e_ld| <= max(16 |e64 - e_ld|, 64 eps y2),      e64 = y2 - 2 beta . qv + beta^T Qm beta in float64
  h_{f,s}        |h - h_ld| <= max(16 |h64 - h_ld|, 64 eps bb_f),    h64 = bb_f - 2 beta . c_f + beta^T G_f beta in float64
16: the left-looking recurrence adds up to S further roundings per entry in another order than LAPACK's.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import lasso_path as lp  # noqa: E402

LD = np.longdouble
EPS = np.finfo(np.float64).eps
PIVOT_TOL = LD(1e-10)
MIN_MARGIN = 1e-6
BAR_FACTOR = 16
NCONF, PER_CONF, NCLASS = 60, 25, 3


@functools.lru_cache(maxsize=None)
def rows(seed, K, nconf=NCONF, per=PER_CONF):
    """(A, b, w, configuration per row, class per row): columns scaled over six decades, a sparse truth (about a quarter of
    the columns, at least one) plus noise, weights in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    m = nconf * per
    scale = 10.0 ** rng.uniform(-3.0, 3.0, K)
    A = rng.standard_normal((m, K)) * scale
    truth = np.where(rng.random(K) < 0.25, rng.standard_normal(K) * rng.uniform(0.3, 3.0, K), 0.0) / scale
    if not truth.any():
        truth[0] = 1.0 / scale[0]
    b = A @ truth + 0.1 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    conf = np.repeat(np.arange(nconf), per).astype(np.int64)
    cls = (np.arange(m) % NCLASS).astype(np.int64)
    for x in (A, b, w, conf, cls):
        x.setflags(write=False)
    return A, b, w, conf, cls


def fold_of_conf(conf, F):
    """Configurations dealt round-robin into F folds."""
    return conf % F


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


@functools.lru_cache(maxsize=None)
def case_blocks(seed, K, F, nsub=1):
    """The rows of ``rows(seed, K)`` and their F * nsub blocks (category = fold * nsub + class for nsub = 3)."""
    A, b, w, conf, cls = rows(seed, K)
    fold = fold_of_conf(conf, F)
    cat = fold * nsub + (cls if nsub > 1 else 0)
    blocks = blocks_ld(A, b, w, cat, F * nsub)
    blocks.setflags(write=False)
    return blocks


def edge_rows(F):
    """K = 12 rows in F folds: column 3 is zero, fold 1 alone touches column 7, column 5 is twice column 2.  (K, A, b, w, fold)"""
    K = 12
    A, b, w, conf, _ = rows(7, K)
    A, b = A.copy(), b.copy()
    fold = fold_of_conf(conf, F)
    A[:, 3] = 0.0
    A[fold != 1, 7] = 0.0
    A[:, 5] = 2.0 * A[:, 2]
    b = b + 0.5 * A[:, 7] / np.abs(A[:, 7]).max()
    return K, A, b, w, fold


def omp_ld(Qm, qv, y2, tdiag, criterion, forced, S):
    """The yardstick: (order (S), e (S), coef (S x K), margin (S)) in long double; margin[s] is (best - second best) / best
    of the scores at a step that took the argmax among at least two candidates, inf elsewhere."""
    Q, q = np.asarray(Qm, dtype=LD), np.asarray(qv, dtype=LD)
    K = q.shape[0]
    qd0 = np.diag(Q).copy()
    ref = qd0 if tdiag is None else np.asarray(tdiag, dtype=LD)
    alive = ~((ref == 0) | (qd0 <= PIVOT_TOL * ref))
    cand = alive.copy()
    qd = np.where(alive, qd0, LD(0))
    t, r = qd.copy(), np.where(alive, q, LD(0))
    W = np.zeros((S, K), dtype=LD)
    z = np.zeros(S, dtype=LD)
    order = np.full(S, -1, dtype=np.int64)
    e_out, coef, margin = np.zeros(S, dtype=LD), np.zeros((S, K), dtype=LD), np.full(S, np.inf)
    e, ns, fpos = LD(y2), 0, 0
    forced = [int(j) for j in forced]
    ended = False
    for s in range(S):
        js = -1
        if not ended:
            cand &= ~(cand & (t <= PIVOT_TOL * qd))
            while fpos < len(forced) and js < 0:
                j = forced[fpos]
                fpos += 1
                if cand[j]:
                    js = j
            if js < 0 and cand.any():
                idx = np.flatnonzero(cand)
                sc = r[idx] * r[idx] / (t[idx] if criterion == "ols" else qd[idx])
                k = int(np.argmax(sc))                       # the first of equal maxima: the lowest index
                js = int(idx[k])
                if len(idx) > 1:
                    rest = np.delete(sc, k)
                    margin[s] = float((sc[k] - rest.max()) / sc[k]) if sc[k] > 0 else 0.0
            if js < 0:
                ended = True
        if js >= 0:
            l = np.sqrt(t[js])
            wk = np.where(alive, (Q[js] - W[:ns, js] @ W[:ns]) / l, LD(0))
            z[ns] = r[js] / l
            r = r - wk * z[ns]
            t = t - wk * wk
            e = e - z[ns] * z[ns]
            W[ns] = wk
            cand[js] = False
            order[s] = js
            ns += 1
            x = z[:ns].copy()
            for v in range(ns - 1, -1, -1):
                jv = order[v]
                x[v] = x[v] / W[v, jv]
                x[:v] -= W[:v, jv] * x[v]
            coef[s, order[:ns]] = x
        elif s > 0:
            coef[s] = coef[s - 1]
        e_out[s] = e
    return order, e_out, coef, margin


def bars(Qm, qv, y2, order, coef_ld, e_ld):
    """(coefficient bar (S), e bar (S)) of the module docstring for one problem; 64 eps floors where the path took no step."""
    S = len(order)
    cb, eb = np.zeros(S), np.zeros(S)
    ns = 0
    for s in range(S):
        if order[s] >= 0:
            ns = s + 1
        sup = np.asarray(order[:ns], dtype=np.int64)
        beta_ld = coef_ld[s]
        err64 = 0.0
        if ns:
            b64 = np.linalg.solve(Qm[np.ix_(sup, sup)], qv[sup])
            err64 = float(np.max(np.abs(np.asarray(b64, dtype=LD) - beta_ld[sup])))
        cb[s] = max(BAR_FACTOR * err64, 64 * EPS * float(np.max(np.abs(beta_ld))))
        b = beta_ld.astype(np.float64)
        e64 = y2 - 2.0 * (b @ qv) + b @ (Qm @ b)
        eb[s] = max(BAR_FACTOR * abs(float(LD(e64) - e_ld[s])), 64 * EPS * y2)
    return cb, eb


def heldout_ld(block, K, coef_ld):
    """(h_ld (S), bar (S)) of fold ``block`` under the yardstick's coefficients."""
    G, c, bb, _ = lp.unpack(block, K)
    GL, cL = np.asarray(G, dtype=LD), np.asarray(c, dtype=LD)
    h_ld = np.array([LD(bb) - 2 * (x @ cL) + x @ (GL @ x) for x in coef_ld], dtype=LD)
    b64 = coef_ld.astype(np.float64)
    h64 = bb - 2.0 * (b64 @ c) + np.einsum("sk,sk->s", b64 @ G, b64)
    bar = np.maximum(BAR_FACTOR * np.abs((np.asarray(h64, dtype=LD) - h_ld).astype(np.float64)), 64 * EPS * bb)
    return h_ld, bar


def sklearn_supports(Qm, qv, y2, steps):
    """The supports (sets of columns) after 1 ... steps steps of scikit-learn's orthogonal_mp_gram on the column-normalised
    system (every column of Qm must be live)."""
    from sklearn.linear_model import orthogonal_mp_gram

    d = np.sqrt(np.diag(Qm))
    path = orthogonal_mp_gram(Qm / d[:, None] / d[None, :], qv / d, n_nonzero_coefs=int(steps), norms_squared=np.array([float(y2)]),
                              copy_Gram=True, copy_Xy=True, return_path=True)
    path = np.asarray(path).reshape(Qm.shape[0], -1)
    return [set(np.flatnonzero(path[:, s]).tolist()) for s in range(path.shape[1])]


def stepwise_rows(X, y, steps, forced=()):
    """Brute-force forward stepwise regression on the rows: at every step the column whose least-squares refit together with
    the chosen ones leaves the smallest residual sum of squares.  The order."""
    K = X.shape[1]
    chosen = []
    forced = list(forced)
    for _ in range(steps):
        if forced:
            chosen.append(forced.pop(0))
            continue
        best, bj = np.inf, -1
        for j in range(K):
            if j in chosen:
                continue
            cols = chosen + [j]
            res = y - X[:, cols] @ np.linalg.lstsq(X[:, cols], y, rcond=None)[0]
            rss = float(res @ res)
            if rss < best:
                best, bj = rss, j
        chosen.append(bj)
    return chosen


def check_problem(Qm, qv, y2, tdiag, criterion, forced, S, order, path, coef, where=""):
    """One problem of the code under test against the yardstick: equal order, e_s and coefficients within the bars, a margin
    of at least MIN_MARGIN at every step.  ``coef``: (S x K), or a dict {level: row}.  Returns (worst coefficient error / bar,
    worst e error / bar, smallest margin, the yardstick's coefficients)."""
    o_ld, e_ld, c_ld, margin = omp_ld(Qm, qv, y2, tdiag, criterion, forced, S)
    assert margin.min() >= MIN_MARGIN, (where, "margin", margin.min())
    assert np.array_equal(np.asarray(order, dtype=np.int64), o_ld), (where, order, o_ld)
    cb, eb = bars(Qm, qv, y2, o_ld, c_ld, e_ld)
    e_err = np.abs((np.asarray(path[:, 0], dtype=LD) - e_ld).astype(np.float64))
    print(f"{where}: e_s worst error / bar {np.max(e_err / eb):.3f}", flush=True)
    assert np.all(e_err <= eb), (where, "e_s", float(np.max(e_err / eb)))
    levels = coef.keys() if isinstance(coef, dict) else range(1, S + 1)
    worst = 0.0
    for lv in levels:
        got = coef[lv] if isinstance(coef, dict) else coef[lv - 1]
        err = float(np.max(np.abs((np.asarray(got, dtype=LD) - c_ld[lv - 1]).astype(np.float64))))
        worst = max(worst, err / cb[lv - 1])
        sup = o_ld[:lv][o_ld[:lv] >= 0]
        off = np.ones(len(got), dtype=bool)
        off[sup] = False
        assert np.all(np.asarray(got)[off] == 0.0), (where, lv, "a coefficient off the support is not an exact zero")
    print(f"{where}: coefficients worst error / bar {worst:.3f}  smallest margin {margin.min():.2e}", flush=True)
    assert worst <= 1.0, (where, "coefficients", worst)
    return worst, float(np.max(e_err / eb)), float(margin.min()), c_ld
