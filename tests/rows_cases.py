"""References, a-priori bars, inputs and a faulty float64 mirror for the row-streaming kernels of fsnap_rows.hip
(kernel 3 weight_rows, kernel 4 gemv_rows, kernel 7 gemvT_rows + colsum, kernel 4+7 residual_rows, kernel 9 error_stats),
shared by tests/test_rows_cases_cpu.py and tests/test_gpu_rows.py.  Pure numpy.

References are evaluated in ``np.longdouble`` (64-bit mantissa, eps 1.1e-19: three decimal digits below every bar here).

Bars
----
First-order forward-error bounds of a float64 evaluation that hold for ANY summation order (a sum of n terms in any
tree has at most n - 1 roundings on the path of a term).  They depend on the data and the long-double reference only,
never on the kernel's output or on its summation tree.  Notation: u = 2^-53, gamma_n = n u / (1 - n u), K columns,
m_t = number of training rows (mask set) with non-zero weight; all sums over i run over those rows (any other row
contributes an exact zero), p_i, r_i = b_i - p_i are the long-double values.

  aw, bw       no bar: aw_ik = fl(w_i a_ik), bw_i = fl(w_i b_i), one IEEE multiply -- equal to the float64 product bit for
               bit; rows with the mask clear are exactly +0.0.
  p_i = a_i.beta
               delta_i = gamma_{K+1} sum_k |a_ik| |beta_k|          (K products, K - 1 additions, fused or not)
  s_c = sum_i a_ic w_i^2 r_i
               sum_i |a_ic| w_i^2 (delta_i + 3u |r_i|)               error of p_i; subtraction and two multiplies of u_i
               + gamma_{m_t+3} sum_i |a_ic| w_i^2 |r_i|              product and the sum over the rows, in any order
  sse = sum_i (w_i r_i)^2
               sum_i 2 |w_i r_i| w_i (delta_i + 2u |r_i|)            error of p_i; subtraction and multiply of w_i r_i
               + gamma_{m_t+2} sse                                   square and the sum over the rows

Error statistics of a category with n_c rows (all of its rows: the weights of kernel 9 are not masked), n_w of them with a
non-zero weight, t = truth, r = t - p, mean = sum t / n_c, wmean = sum w t / n_w (0 when n_w = 0) -- the ten columns of
fsnap_error_stats: [n_c, n_w, sum t, sum w t, sum |r|, sum r^2, sum (t - mean)^2, sum |w r|, sum (w r)^2,
sum (w t - wmean)^2].  The LDS atomics add in no fixed order: the any-order bound is the right one, and no run-to-run bit
identity is asserted.

  n_c, n_w     exact
  sum t        gamma_{n_c} sum |t|
  sum w t      gamma_{n_c} sum |w t|                                  (product + n_c - 1 additions)
  the means    e_mean  = gamma_{n_c} sum |t| / n_c + u |mean|         (error of the sum, one division)
               e_wmean = gamma_{n_c} sum |w t| / n_w + u |wmean|
  every sum of pass 1 is  sum_i f(x_i)  of an argument x_i that carries a propagated error e_i:
               sum_i |f'(x_i)| e_i + gamma_{n_c+1} sum_i |f(x_i)|     (f = |.| or the square: one product, n_c - 1 additions)
  with         x = r:            e_i = delta_i + u |r_i|
               x = t - mean:     e_i = e_mean + u |t_i - mean|
               x = w r:          e_i = w_i (delta_i + 2u |r_i|)
               x = w t - wmean:  e_i = u |w_i t_i| + e_wmean + u |w_i t_i - wmean|
  and |f'| = 1 for |.|, 2 |x_i| for the square.

Inputs
------
``make_case``: A = standard_normal x uniform(0.5, 2) per column; w exactly 0 for 10 % of the rows, otherwise
uniform(0.5, 2) -- NOT spread over decades: a dropped row of weight 1e-3 hides under the bar of s; a 20 % testing mask;
b = A x + noise + 3; beta random and far from x, so that no row's residual is small.  The last row and the first row of the
last 32-row block are training rows of non-zero weight and one row in the middle is a test row of non-zero weight, so that
every fault of the mirror below has something to move.  ``make_stats_case``: truth with mean 1000 and spread 50, random
category ids including -1 and ids >= ncat (ignored), and -- from four categories on -- an empty category, a one-row
category and a category whose weights are all zero.

Mirror
------
``mirror`` / ``stats_mirror`` evaluate the same operations in float64 numpy, with one switchable fault each (``FAULTS``,
``STATS_FAULTS``): tests/test_rows_cases_cpu.py shows that the fault-free mirror stays within 1.0 bars, that every fault
lands more than 100 bars outside, and that every bar is at most 1e-9 of the sum of the absolute terms of its quantity --
which keeps the GPU assertions from being vacuous."""
import functools
import types

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# ---- shapes of the GPU sweeps (tests/test_gpu_rows.py; tests/test_rows_cases_cpu.py checks the bars on the same ones) ----
# both sides of every switch of the launchers: lane widths 4 / 8 / 16 / 32 / 64 of kernels 3 and 7 (K <= 8, 16, 32, 64), their
# second column pass (K > 128), the 32-column steps NJ = 1 ... 9 of kernel 4+7, its end at 288, the LDS limit of kernel 7
K_SWEEP = (1, 2, 7, 8, 9, 16, 17, 31, 32, 33, 64, 65, 127, 128, 129, 192, 193, 224, 225, 256, 257, 288, 289, 511, 1595)
M_SWEEP = (1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 257)
M_SWEEP_K = (31, 129)
# grid caps: kernels 4 and 4+7 (NJ = 1) loop beyond 65536 rows, kernel 4+7 with NJ = 9 beyond 16384; kernel 7 has 2048
# workgroups of rows_per_wg = ceil(m / 2048) rows: at m = 131073 that is 65 and the last workgroups start past m
GRID_CASES = ((65535, 4), (65537, 4), (65536 + 33, 4), (16384 + 33, 288), (131073, 4))
LAYOUT_CASES = ((31, 36), (31, 32), (32, 37), (32, 33), (129, 134), (129, 130), (288, 293), (288, 289), (300, 305), (300, 301))
LAYOUT_M = 1003
GARBAGE_K = (31, 129, 288, 300, 448)
GARBAGE_M = 2003
FUSED_MAX_K = 288
# (m, K, ncat); the last one is the grid-stride loop of kernel 9 (512 workgroups x 16 x 256 rows)
STATS_CASES = ((5003, 5, 1), (20011, 5, 37), (20011, 5, 3000), (512 * 4096 + 4097, 1, 37))
STATS_MAX_NCAT = 3000


def sweep_m(K):
    """Rows of the K sweep: a few thousand, odd, more than one workgroup of every kernel."""
    return 3003 if K <= FUSED_MAX_K else 2051


def need_long_double():
    if np.finfo(LD).eps > 2e-19:
        raise RuntimeError(f"np.longdouble has eps = {np.finfo(LD).eps}: the references of the row kernels need an "
                           "extended-precision long double (eps <= 2e-19)")


def gamma(n):
    n = np.asarray(n, dtype=LD)
    return n * U / (1 - n * U)


# ---- inputs ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def make_case(m, K, lda=None, masked=True, seed=None):
    """Rows (m x K inside an m x lda buffer ``big`` whose padding columns are NaN), b, w, the training mask (None: no
    mask at all) and beta.  Cached: the arrays are shared and must not be written to."""
    rng = np.random.default_rng(1000003 * K + m if seed is None else seed)
    lda = K if lda is None else lda
    big = np.full((m, lda), np.nan)
    big[:, :K] = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    A = big[:, :K]
    w0 = rng.uniform(0.5, 2.0, m)
    w = np.where(rng.random(m) < 0.1, 0.0, w0)
    train = rng.random(m) >= 0.2
    last, block = m - 1, (m - 1) // 32 * 32
    test_row = None
    for r in (last, block):
        train[r] = True
        w[r] = w0[r]
    if m >= 3:
        test_row = m // 2 if m // 2 not in (last, block) else m // 2 - 1
        if test_row in (last, block):
            test_row = None
        else:
            train[test_row] = False
            w[test_row] = w0[test_row]
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m) + 3.0
    beta = rng.standard_normal(K)
    for a in (big, b, w, train, beta):
        a.setflags(write=False)
    c = types.SimpleNamespace(name=f"{m}x{K}" + (f" lda={lda}" if lda != K else "") + ("" if masked else " no mask"),
                              m=m, K=K, lda=lda, big=big, A=A, b=b, w=w, mask=train if masked else None, beta=beta,
                              test_row=test_row if masked else None, last_row=last, block_row=block,
                              key=(m, K, None if lda == K else lda, masked, seed))
    return c


def keep_rows(case):
    return np.ones(case.m, dtype=bool) if case.mask is None else case.mask


def with_garbage(case):
    """(big, b, w) with NaN in A, Inf in b and -Inf in w of every test row."""
    t = ~keep_rows(case)
    big, b, w = case.big.copy(), case.b.copy(), case.w.copy()
    big[t] = np.nan
    b[t] = np.inf
    w[t] = -np.inf
    return big, b, w


@functools.lru_cache(maxsize=None)
def make_stats_case(m, K, ncat, seed=None):
    rng = np.random.default_rng(77 * ncat + m if seed is None else seed)
    A = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    w = np.where(rng.random(m) < 0.1, 0.0, rng.uniform(0.5, 2.0, m))
    t = 1000.0 + 50.0 * rng.standard_normal(m)
    beta = rng.standard_normal(K)
    cat = rng.integers(-1, ncat + 2, size=m).astype(np.int32)       # -1, ncat and ncat + 1: rows of no category
    empty = single = zero_w = None
    if ncat >= 4:
        empty, single, zero_w = 1, 2, 3
        cat[cat == empty] = -1
        cat[cat == single] = ncat + 1
        cat[m // 3] = single
        cat[[m // 5, m // 7]] = zero_w
        w[cat == zero_w] = 0.0
    drop_cat = 0
    assert np.count_nonzero(cat == drop_cat) >= 2
    for a in (A, w, t, beta, cat):
        a.setflags(write=False)
    return types.SimpleNamespace(name=f"{m}x{K} ncat={ncat}", m=m, K=K, ncat=ncat, A=A, b=t, w=w, beta=beta, cat=cat,
                                 empty=empty, single=single, zero_w=zero_w, drop_cat=drop_cat, key=(m, K, ncat, seed))


# ---- long-double references and bars ---------------------------------------------------------------------------------------

def _predictions(A, beta):
    """(p, delta) in long double: p = A beta and its bar."""
    need_long_double()
    K = A.shape[1]
    Al = A.astype(LD)
    p = Al @ beta.astype(LD)
    delta = gamma(K + 1) * (np.abs(Al) @ np.abs(beta).astype(LD))
    return Al, p, delta


def reference(case):
    """Long-double values and bars of a case of ``make_case``, computed once per case (cached on the case's arguments): aw,
    bw (float64, exact), p, p_bar, p_terms, s, s_bar, s_terms, sse, sse_bar."""
    return _reference(case.key)


@functools.lru_cache(maxsize=None)
def _reference(key):
    case = make_case(*key)
    keep = keep_rows(case)
    Al, p, delta = _predictions(case.A, case.beta)
    wk = np.where(keep, case.w, 0.0).astype(LD)
    r = case.b.astype(LD) - p
    wr = wk * r
    u = wk * wr
    mt = int(np.count_nonzero(keep & (case.w != 0.0)))
    absA = np.abs(Al)
    s_terms = np.abs(u) @ absA
    s_bar = (wk * wk * (delta + 3 * U * np.abs(r))) @ absA + gamma(mt + 3) * s_terms
    sse = np.sum(wr * wr)
    sse_bar = np.sum(2 * np.abs(wr) * wk * (delta + 2 * U * np.abs(r))) + gamma(mt + 2) * sse
    return types.SimpleNamespace(
        aw=np.where(keep[:, None], case.w[:, None] * case.A, 0.0), bw=np.where(keep, case.w * case.b, 0.0),
        p=p, p_bar=delta, p_terms=delta / gamma(case.K + 1), s=u @ Al, s_bar=s_bar, s_terms=s_terms, sse=sse, sse_bar=sse_bar)


def _group_sum(cat, ncat, vals):
    out = np.zeros(ncat, dtype=LD)
    np.add.at(out, cat, vals)
    return out


def stats_reference(case):
    """(ref, bar, terms): three (ncat, 10) long-double tables -- the statistics, their bars and the sums of the absolute
    terms (the counts have bar 0).  Cached for the cases of ``make_stats_case``; any other object with the same fields
    (A, b, w, beta, cat, ncat) is evaluated directly."""
    key = getattr(case, "key", None)
    return compute_stats_reference(case) if key is None else _stats_reference(key)


@functools.lru_cache(maxsize=None)
def _stats_reference(key):
    return compute_stats_reference(make_stats_case(*key))


def compute_stats_reference(case):
    ncat = case.ncat
    _, p, delta = _predictions(case.A, case.beta)
    ok = (case.cat >= 0) & (case.cat < ncat)
    cat = case.cat[ok]
    t, w, p, delta = case.b[ok].astype(LD), case.w[ok].astype(LD), p[ok], delta[ok]
    gs = functools.partial(_group_sum, cat, ncat)
    n, nw = gs(np.ones(len(cat), dtype=LD)), gs((w != 0).astype(LD))
    wt = w * t
    st, swt, sat, sawt = gs(t), gs(wt), gs(np.abs(t)), gs(np.abs(wt))
    mean = np.where(n > 0, st / np.maximum(n, 1), 0)
    wmean = np.where(nw > 0, swt / np.maximum(nw, 1), 0)
    gn, g1 = gamma(n), gamma(n + 1)
    e_mean = gn * sat / np.maximum(n, 1) + U * np.abs(mean)
    e_wmean = np.where(nw > 0, gn * sawt / np.maximum(nw, 1), 0) + U * np.abs(wmean)
    r = t - p
    wr = w * r
    dt, dwt = t - mean[cat], wt - wmean[cat]
    e_r = delta + U * np.abs(r)
    e_dt = e_mean[cat] + U * np.abs(dt)
    e_wr = w * (delta + 2 * U * np.abs(r))
    e_dwt = U * np.abs(wt) + e_wmean[cat] + U * np.abs(dwt)
    ref, bar, terms = (np.zeros((ncat, 10), dtype=LD) for _ in range(3))
    ref[:, 0], ref[:, 1] = n, nw
    terms[:, 0], terms[:, 1] = n, nw
    ref[:, 2], bar[:, 2], terms[:, 2] = st, gn * sat, sat
    ref[:, 3], bar[:, 3], terms[:, 3] = swt, gn * sawt, sawt
    for col, x, e, square in ((4, r, e_r, False), (5, r, e_r, True), (6, dt, e_dt, True), (7, wr, e_wr, False),
                              (8, wr, e_wr, True), (9, dwt, e_dwt, True)):
        f = x * x if square else np.abs(x)
        d = 2 * np.abs(x) if square else 1.0
        ref[:, col] = terms[:, col] = gs(f)
        bar[:, col] = gs(d * e) + g1 * ref[:, col]
    return ref, bar, terms


# ---- error / bar ----------------------------------------------------------------------------------------------------------

def worst(got, ref, bar):
    """max |got - ref| / bar; a zero bar admits a zero error only (then the ratio is 0, otherwise inf), a non-finite value
    is inf."""
    got, ref, bar = (np.atleast_1d(np.asarray(a, dtype=LD)) for a in (got, ref, bar))
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.inf))
    return float(np.max(ratio))


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def score(case, out, rows=None):
    """Worst error / bar of each output in ``out`` (keys of aw, bw, p, sse, s; aw and bw: 0 when bit-identical to the
    float64 product, inf otherwise).  ``rows``: compare the predictions of these rows only."""
    ref = reference(case)
    res = {}
    for k in ("aw", "bw"):
        if k in out:
            res[k] = 0.0 if same_bits(out[k], getattr(ref, k)) else np.inf
    if "p" in out:
        sel = slice(None) if rows is None else rows
        res["p"] = worst(np.asarray(out["p"])[sel], ref.p[sel], ref.p_bar[sel])
    if "sse" in out:
        res["sse"] = worst(out["sse"], ref.sse, ref.sse_bar)
    if "s" in out:
        res["s"] = worst(out["s"], ref.s, ref.s_bar)
    return res


def stats_score(case, got):
    """Worst error / bar over the categories of each of the ten columns."""
    ref, bar, _ = stats_reference(case)
    return [worst(np.asarray(got)[:, c], ref[:, c], bar[:, c]) for c in range(10)]


# ---- float64 mirror with switchable faults ----------------------------------------------------------------------------------

FAULTS = ("drop_last_row", "drop_block_row", "drop_last_column", "odd_neighbour", "ignore_mask", "w_for_w2")
STATS_FAULTS = ("drop_category_row",)


def applicable(case, fault):
    if fault == "odd_neighbour":
        return case.K % 2 == 1 and case.m >= 2
    if fault == "ignore_mask":
        return case.test_row is not None
    return True


def mirror(case, fault=None):
    """aw, bw, p, sse, s in float64 numpy.  Faults: the last row / the first row of the last 32-row block is never
    processed; the last column is left out; the upper half of an odd-width row's last 16-byte pair (its neighbour's first
    element) is not selected away: it enters the prediction with the last column's coefficient beta[K - 1] and is written,
    weighted with this row's w, over the neighbour's first element of aw; the mask of one test row is ignored; u = w r instead of w^2 r."""
    assert fault is None or (fault in FAULTS and applicable(case, fault))
    m, K = case.m, case.K
    A, b, w, beta = np.array(case.A), case.b, case.w, case.beta
    keep = keep_rows(case).copy()
    done = np.ones(m, dtype=bool)
    if fault == "drop_last_row":
        done[case.last_row] = False
    if fault == "drop_block_row":
        done[case.block_row] = False
    if fault == "ignore_mask":
        keep[case.test_row] = True
    if fault == "drop_last_column":
        A[:, K - 1] = 0.0
    keep &= done
    p = A @ beta
    aw = np.where(keep[:, None], w[:, None] * A, 0.0)
    bw = np.where(keep, w * b, 0.0)
    if fault == "odd_neighbour":
        p[:-1] += A[1:, 0] * beta[K - 1]
        aw[1:, 0] = np.where(keep[:-1], w[:-1] * A[1:, 0], aw[1:, 0])
    p[~done] = 0.0
    wk = np.where(keep, w, 0.0)
    r = wk * (b - p)
    u = r if fault == "w_for_w2" else wk * r
    return {"aw": aw, "bw": bw, "p": p, "sse": float(r @ r), "s": u @ A}


def stats_mirror(case, fault=None):
    """The (ncat, 10) table in float64 numpy; fault: the last row of category ``case.drop_cat`` is left out."""
    assert fault is None or fault in STATS_FAULTS
    ncat = case.ncat
    ok = (case.cat >= 0) & (case.cat < ncat)
    if fault == "drop_category_row":
        ok[np.flatnonzero(case.cat == case.drop_cat)[-1]] = False
    cat = case.cat[ok]
    t, w = case.b[ok], case.w[ok]
    r = t - (case.A @ case.beta)[ok]
    gs = lambda v: np.bincount(cat, weights=v, minlength=ncat)
    out = np.zeros((ncat, 10))
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = gs(np.ones(len(cat))), gs((w != 0) * 1.0), gs(t), gs(w * t)
    mean = np.where(out[:, 0] > 0, out[:, 2] / np.maximum(out[:, 0], 1), 0.0)
    wmean = np.where(out[:, 1] > 0, out[:, 3] / np.maximum(out[:, 1], 1), 0.0)
    wr = w * r
    for col, v in ((4, np.abs(r)), (5, r * r), (6, (t - mean[cat]) ** 2), (7, np.abs(wr)), (8, wr * wr),
                   (9, (w * t - wmean[cat]) ** 2)):
        out[:, col] = gs(v)
    return out
