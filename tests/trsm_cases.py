"""Reference, a-priori bars, inputs and a faulty float64 mirror for ONE pass Q <- X R^-1 of the row-space solve (kernels 13C
``fsnap_trsm_acc2_k<NB, FIRST>`` and 13B ``fsnap_trsm_panel_k<TR, KG, FIRST>`` of fsnap_trsm.hip), shared by
tests/test_trsm_cases_cpu.py and tests/test_gpu_trsm.py.  Pure numpy.

Reference
---------
Q* = X R^-1 by column substitution in ``np.longdouble`` (64-bit mantissa, eps 1.1e-19), vectorised over the rows:
q_j = (x_j - sum_{i<j} q_i r_ij) / r_jj.  For a first pass X is the product w_i a_ik formed in long double (NOT the float64
product: the kernel's rounding of w a is part of what the bars allow); rows with w_eff = 0 (mask clear or zero weight) are
exact +0.0 whatever A holds there.  Its own error, gamma_K in long double, is 2^-11 of the bars below.

Bars
----
First order, from the data and the long-double reference only, never from the kernel's output.  u = 2^-53,
gamma_n = n u / (1 - n u); q is the kernel's row, q* the reference row, x the row of X:

  backward, per entry   |(q R - x)_j|  <=  gamma_{K+3} (|q*| |R|)_j
  forward, per entry    |(q - q*)_j|   <=  gamma_{K+3} (|q*| |R| |R^-1|)_j

K + 3 counts: the substitution in ANY accumulation order -- (R + dR) q = x with |dR| <= gamma_K |R| (Higham, Accuracy and
Stability of Numerical Algorithms, Thm 8.5; the order of the sum over i is free, so the MFMA updates, the left- and
right-looking structure and fused multiply-adds are all covered); one more rounding for the multiplication by fl(1 / r_jj)
where the reference divides; one for the first pass's fl(w a), which the compiler may or may not fuse into the following
subtraction; one of slack for the first-order step (q for q* on the right-hand sides).  The forward bar is the backward one
pushed through |R^-1|: q - q* = (x - q* R + q R - x) R^-1 = (q R - x) R^-1.
The backward residual of the kernel's q is evaluated in long double (rounding 2^-11 of the bar).  |q*| |R| and its product
with |R^-1| are sums of non-negative terms and are evaluated in float64 (relative error gamma_K, 1e-13: not inflated for);
R^-1 itself is computed in long double.

Kernel 13B multiplies by the float64 inverse T^-1 of each 16 x 16 diagonal block T and refines once (q0 = x T^-1,
r = x - q0 T, q = q0 + r T^-1): its residual carries an extra cond(T)^2 u^2 term next to the cond-free gamma |q| |T| of a
substitution, below u for cond(T) <~ 1e7.  It is held to the SAME bars; the factors below keep cond(T) of every block that
kernel 13B meets (K >= 129) under 1e7 (``Factor.cond_t``, asserted by the CPU test, listed in profiles/trsm_accuracy.txt).

Rows beyond the long-double budget: while m K^2 <= 1e8 every row gets both bars.  Above, the long-double check runs on the
rows of the first and of the last 64-row tile and on every 7th row; the rest is
held to the float64 residual |q R - x| <= 2 gamma_{K+3} (|q~| |R|) with q~ a float64 substitution (LAPACK trsm) standing in
for q* -- the second bar covers the float64 evaluation's own rounding (gamma_K |q| |R|).

Factors (``factor``)
--------------------
  benign    diagonal 2 + 0.1 N(0,1), off-diagonal 0.1 N(0,1) / sqrt(K)  (what tools/trsm_check uses)
  illblock  every 16 x 16 diagonal block T is the R factor (positive diagonal) of a matrix with singular values
            logspace(0, -4); R = blockdiag(T) (I + N) with N strictly block upper, 0.1 N(0,1) / sqrt(K): the blocks are
            ill-conditioned, the coupling between them is not, so R^-1 does not grow with the number of blocks
  cholqr    what fsnap_lstsq_rows feeds the kernel: the Cholesky factor of the Gram matrix of rows with singular values
            logspace(0, -6) (kappa 1e6) whose columns are graded from 1e3 down to 1e-3; formed as the R factor of
            S V^T D.  The rows X of these cases lie in its row space (X = G S V^T D, G standard normal, so that
            Q* = G Q_r is of order one): the forward bar is loose there (|R| |R^-1| ~ kappa), the backward bar counts.

Inputs (``make_case``)
----------------------
benign / illblock: X standard normal, scaled per column by uniform(0.5, 2).  Weights uniform(0.5, 2) with 10 % exact zeros
and a 20 % testing mask; the masked and zero-weight rows of A hold NaN and +-Inf (first pass; a later pass reads the Q of
a first pass, whose rows of zero weight are zero rows: there they ARE zero).  Training rows of non-zero weight by
construction: the last row, the first row of the last 64-row tile, the first and the last row of the first tile.

Mirror (``mirror``)
-------------------
Float64 numpy with the kernels' structure -- 13C: 64-column panels, left-looking over the solved panels, right-looking
inside, substitution with the reciprocal; 13B: 128-column panels, a GEMM over the solved panels, q0 / r / q per block with
the float64 inverse blocks (a port of trsm_invert_diagonal_blocks), right-looking updates -- and one switchable fault per
mechanism the kernels guard by hand (``FAULTS``; ``fault_acts`` says on which shapes a fault can move anything):

  drop_last_update     the update of the last block of the last panel by the block before it is dropped (the wait-state
                       hazard recorded at mfma_settle in fsnap_trsm.hip)
  left_block_off       one left-looking block row of a panel > 0 is taken one block off (rows of R of the next block)
  col_ge_k_next_row    columns >= K of the last block are read from the next row (lda = K) instead of selected to zero.
                       Kernel 13C cannot show it: column j of a substitution never sees a column > j, and the last block
                       feeds no update.  Kernel 13B multiplies the whole block by T^-1: finite garbage meets exact zeros,
                       NaN / Inf of a masked next row does not
  store_ge_k_next_row  a store into a column >= K lands in the next row (its first K16 - K columns; behind the last row)
  ragged_row_stale     the last row of a ragged tile is not stored: it keeps what the buffer held
  zero_weight_multiplied  a row of zero weight is multiplied by it instead of selected away: NaN gets through
  weights_twice        first pass: the weights are applied again to a solved panel that is read back
  inplace_overwritten  a later pass: the second block of a panel (the first when it has one) is read after it was overwritten
  reciprocal_f32       kernel 13C: the reciprocal of the diagonal is rounded to float32 (kernel 13B has no reciprocal: its
                       inverse blocks come from the host, and one refinement step would square the 6e-8 away)

tests/test_trsm_cases_cpu.py shows that the fault-free mirror stays within 1.0 bars on every shape of the GPU sweeps, that
every fault lands more than 100 bars outside on at least one of the two bars wherever it acts, that Q* R gives back X to
long-double rounding, and that the bars are not vacuous: on benign and illblock factors the forward bar of every entry is
at most 1e-9 of the largest |q*| of its row (the backward bar is gamma_{K+3} <= 2e-13 of (|q*| |R|)_j by construction)."""
import functools
import types

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
KINDS = ("benign", "illblock", "cholqr")
FAMILY_13C, FAMILY_13B16, FAMILY_13B32 = 1, 2, 3
LD_BUDGET = 1.0e8          # m K^2 up to which every row is checked in long double
SENTINEL = -1.2345e300     # guard rows around Q, and what Q holds before a first pass
GUARD_ROWS = 64

# ---- shapes of the GPU sweeps ------------------------------------------------------------------------------------------------
# kernel 13C: every NB = 1 ... 9, both panel boundaries (NB = 4 | 5, 8 | 9), a last block of 1 ... 16 columns; three full
# 64-row tiles (the unguarded loads and stores) + a ragged one of 37 rows
C_COLS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 96, 97, 111, 112, 113, 127, 128, 129, 142, 143, 144)
C_COLS_M = 229
C_ROWS_K = (31, 113, 142)
C_ROWS_M = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129)
# kernel 13B: a last panel of 1 ... 8 blocks with 2, 3 and 4 panels, last panels shorter than a 64-row slab, 13 panels
B_COLS = tuple(sorted({k for k16 in range(144, 401, 16) for k in (k16, k16 - 15)} | {512, 513, 1024, 1595}))
B_COLS_M = {FAMILY_13B16: 2 * 64 + 37, FAMILY_13B32: 2 * 128 + 37}
B_ILL_K16 = (208, 256, 272, 400)
B_ROWS_K = (145, 208, 300)
B_ROWS_M = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257)
LAYOUT_K = (31, 113, 142, 208, 300)
LAYOUT_M = 229
# (m, K, the family the rule of launch_trsm_rows names)
DISPATCH = ((32767, 144, FAMILY_13B16), (32768, 144, FAMILY_13C), (32767, 160, FAMILY_13B16), (32768, 160, FAMILY_13B32),
            (229, 128, FAMILY_13C))


def k16_of(K):
    return (K + 15) // 16 * 16


def family_runs(family, K):
    """The widths a family exists for (anything else is an argument error of fsnap_trsm_pass)."""
    return k16_of(K) <= 144 if family == FAMILY_13C else k16_of(K) > 128


def rule(m, K):
    """The family launch_trsm_rows picks."""
    k16 = k16_of(K)
    if k16 <= 128 or (k16 == 144 and m >= 64 * 512):
        return FAMILY_13C
    return FAMILY_13B16 if m < 64 * 512 else FAMILY_13B32


def b_kinds(K):
    return KINDS if k16_of(K) in B_ILL_K16 else ("benign", "cholqr")


def sweep_cases():
    """Every (family, first, kind, m, K) of the column and row sweeps of tests/test_gpu_trsm.py."""
    out = []
    for first in (True, False):
        for K in C_COLS:
            out += [(FAMILY_13C, first, kind, C_COLS_M, K) for kind in KINDS]
        for K in C_ROWS_K:
            out += [(FAMILY_13C, first, kind, m, K) for m in C_ROWS_M for kind in ("benign", "cholqr")]
        for fam in (FAMILY_13B16, FAMILY_13B32):
            for K in B_COLS:
                out += [(fam, first, kind, B_COLS_M[fam], K) for kind in b_kinds(K)]
            for K in B_ROWS_K:
                out += [(fam, first, kind, m, K) for m in B_ROWS_M for kind in ("benign", "cholqr")]
    return out


def instance(family, first, K):
    """Name of the template instance a case runs."""
    f = "true" if first else "false"
    if family == FAMILY_13C:
        return f"fsnap_trsm_acc2_k<{k16_of(K) // 16}, {f}>"
    return f"fsnap_trsm_panel_k<{1 if family == FAMILY_13B16 else 2}, {64 if family == FAMILY_13B16 else 16}, {f}>"


def need_long_double():
    if np.finfo(LD).eps > 2e-19:
        raise RuntimeError(f"np.longdouble has eps = {np.finfo(LD).eps}: the reference of the pass kernels needs an "
                           "extended-precision long double (eps <= 2e-19)")


def gamma(n):
    return n * U / (1 - n * U)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and bool(np.array_equal(x.view(np.int64), y.view(np.int64)))


# ---- factors -------------------------------------------------------------------------------------------------------------------

def _inverse_ld(R):
    """R^-1 of an upper triangular matrix by back substitution in long double (on the transpose, row chunks cut at the
    diagonal: contiguous rows and half the zeros of the triangle skipped)."""
    K = R.shape[0]
    Rl = R.astype(LD)
    Y = np.zeros((K, K), dtype=LD)                 # Y = (R^-1)^T, lower triangular
    for i in range(K - 1, -1, -1):
        Y[i, i] = 1 / Rl[i, i]
        for a in range(i + 1, K, 256):
            b = min(a + 256, K)
            Y[a:b, i] = -(Y[a:b, i + 1:b] @ Rl[i, i + 1:b]) / Rl[i, i]
    return Y.T


@functools.lru_cache(maxsize=6)
def factor(K, kind):
    """R (K x K upper, float64), |R|, cond_t = the largest 2-norm condition of a 16 x 16 diagonal block (|R^-1|: ``abs_inverse``), and for cholqr the map ``rows(G)`` from standard-normal G to rows in the row
    space.  Cached; the arrays are shared and read-only."""
    need_long_double()
    rng = np.random.default_rng(7919 * K + KINDS.index(kind))
    rows = None
    if kind == "benign":
        R = np.triu(0.1 * rng.standard_normal((K, K)) / np.sqrt(K), 1)
        R[np.diag_indices(K)] = 2.0 + 0.1 * rng.standard_normal(K)
    elif kind == "illblock":
        D = np.zeros((K, K))
        for j0 in range(0, K, 16):
            n = min(16, K - j0)
            A, _ = np.linalg.qr(rng.standard_normal((n, n)))
            B, _ = np.linalg.qr(rng.standard_normal((n, n)))
            T = np.linalg.qr((A * np.logspace(0, -4, n)) @ B.T)[1]
            D[j0:j0 + n, j0:j0 + n] = T * np.sign(np.diag(T))[:, None]
        N = 0.1 * rng.standard_normal((K, K)) / np.sqrt(K)
        blk = np.arange(K) // 16
        N[blk[:, None] >= blk[None, :]] = 0.0
        R = np.triu(D @ (np.eye(K) + N))
    else:
        V, _ = np.linalg.qr(rng.standard_normal((K, K)))
        s = np.logspace(0, -6, K)
        d = 10.0 ** (3.0 - 6.0 * np.arange(K) / max(K - 1, 1)) if K > 1 else np.ones(1)
        B = (s[:, None] * V.T) * d[None, :]                       # S V^T D: rows g B have the Gram factor below
        R = np.linalg.qr(B)[1]
        R = np.triu(R * np.sign(np.diag(R))[:, None])
        rows = lambda G: (G * s[None, :]) @ V.T * d[None, :]      # noqa: E731
    return factor_of(R, kind, rows)


def factor_of(R, kind="given", rows=None):
    """The record of ``factor`` for any upper triangular R."""
    need_long_double()
    K = R.shape[0]
    R = np.triu(np.ascontiguousarray(R, dtype=np.float64))
    cond_t = max(np.linalg.cond(R[j:j + 16, j:j + 16]) for j in range(0, K, 16))
    absR = np.abs(R)
    for a in (R, absR):
        a.setflags(write=False)
    return types.SimpleNamespace(K=K, kind=kind, R=R, absR=absR, absinv=None, cond_t=float(cond_t), rows=rows)


def abs_inverse(fac):
    """|R^-1| of a factor (float64 rounding of the long-double inverse), formed when a reference first asks for it."""
    if fac.absinv is None:
        fac.absinv = np.abs(_inverse_ld(fac.R)).astype(np.float64)
        fac.absinv.setflags(write=False)
    return fac.absinv


# ---- inputs --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=16)
def make_case(m, K, kind, first, lda=None):
    """One pass: the factor, and for a first pass the rows A (m x K inside an m x lda buffer ``big`` whose padding columns
    are NaN), b, w, the training mask and w_eff; for a later pass the input X (rows of zero w_eff are zero rows).  Cached:
    the arrays are shared and must not be written to."""
    fac = factor(K, kind)
    rng = np.random.default_rng(1000003 * K + 101 * m + 7 * KINDS.index(kind) + int(first))
    G = rng.standard_normal((m, K))
    X0 = fac.rows(G) if fac.rows is not None else G * rng.uniform(0.5, 2.0, K)
    w = np.where(rng.random(m) < 0.1, 0.0, rng.uniform(0.5, 2.0, m))
    w0 = rng.uniform(0.5, 2.0, m)
    train = rng.random(m) >= 0.2
    forced = sorted({m - 1, (m - 1) // 64 * 64, 0, min(63, m - 1)})
    for r in forced:
        train[r] = True
        w[r] = w0[r]
    weff = np.where(train, w, 0.0)
    dead = weff == 0.0
    b = rng.standard_normal(m) + 3.0
    lda = K if lda is None else lda
    big = np.full((m, lda), np.nan)
    big[:, :K] = X0
    if first:
        junk = np.array([np.nan, np.inf, -np.inf])
        big[dead, :K] = junk[rng.integers(0, 3, size=(int(dead.sum()), K))]
        X = None
    else:
        X = X0.copy()
        X[dead] = 0.0
        X.setflags(write=False)
    for a in (big, b, w, train, weff):
        a.setflags(write=False)
    name = f"{kind} {'first' if first else 'later'} {m}x{K}" + (f" lda={lda}" if lda != K else "")
    return types.SimpleNamespace(name=name, m=m, K=K, kind=kind, first=first, lda=lda, fac=fac, R=fac.R, big=big, A=big[:, :K],
                                 b=b, w=w, mask=train, weff=weff, dead=dead, X=X, forced=forced, refs={})


def first_pass_case(A, b, w, mask, R, name):
    """A first-pass case of given rows, weights, mask (None: none) and factor (the replay of a solver call)."""
    m, K = A.shape
    train = np.ones(m, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    weff = np.where(train, w, 0.0)
    fac = factor_of(R)
    return types.SimpleNamespace(name=name, m=m, K=K, kind="given", first=True, lda=K, fac=fac, R=fac.R, big=A, A=A, b=b, w=w,
                                 mask=train, weff=weff, dead=weff == 0.0, X=None, forced=[], refs={})


def x_float64(case):
    """X as a float64 evaluation forms it: fl(w a) selected to zero where w_eff = 0 (first pass), the input otherwise."""
    if not case.first:
        return case.X
    with np.errstate(invalid="ignore"):
        return np.where(case.dead[:, None], 0.0, case.weff[:, None] * case.A)


def sample_rows(m, K, tile=64):
    """(rows checked in long double, the rest): everything while m K^2 <= LD_BUDGET, else the first and the last tile and
    every 7th row."""
    if m * K * K <= LD_BUDGET:
        return np.arange(m), np.arange(0)
    pick = np.zeros(m, dtype=bool)
    pick[:tile] = True
    pick[(m - 1) // tile * tile:] = True
    pick[::7] = True
    return np.flatnonzero(pick), np.flatnonzero(~pick)


# ---- long-double reference and bars --------------------------------------------------------------------------------------------

def _substitute_ld(X, R):
    Rl = R.astype(LD)
    Q = np.empty_like(X)
    for j in range(R.shape[0]):
        s = X[:, j] - Q[:, :j] @ Rl[:j, j] if j else X[:, 0]
        Q[:, j] = s / Rl[j, j]
    return Q


def reference(case, tile=64):
    """Long-double X and Q* of the sampled rows, both bars (float64), and for the rest of the rows the float64 X and bar.
    Computed once per case and tile (kept on the case)."""
    if tile not in case.refs:
        case.refs[tile] = _reference(case, tile)
    return case.refs[tile]


def _reference(case, tile):
    need_long_double()
    fac, K = case.fac, case.K
    rows, rest = sample_rows(case.m, K, tile)
    if case.first:
        with np.errstate(invalid="ignore"):
            x = np.where(case.dead[rows, None], LD(0), case.weff[rows, None].astype(LD) * case.A[rows].astype(LD))
    else:
        x = case.X[rows].astype(LD)
    q = _substitute_ld(x, case.R)
    terms = np.abs(q).astype(np.float64) @ fac.absR                   # (|q*| |R|)_j
    bw_bar = gamma(K + 3) * terms
    fw_bar = gamma(K + 3) * (terms @ abs_inverse(fac))
    out = types.SimpleNamespace(rows=rows, rest=rest, x=x, q=q, terms=terms, bw_bar=bw_bar, fw_bar=fw_bar, rest_x=None, rest_bar=None)
    if rest.size:
        import scipy.linalg

        xr = x_float64(case)[rest]
        qr = scipy.linalg.solve_triangular(case.R, xr.T, trans="T", lower=False).T
        out.rest_x, out.rest_bar = xr, gamma(K + 3) * (np.abs(qr) @ fac.absR)
    return out


def _fraction(err, bar):
    """Largest err / bar and where; a zero bar demands a zero error, NaN counts as infinite."""
    err = np.asarray(err, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0.0, 0.0, err / bar)
    f = np.where(np.isnan(f), np.inf, f)
    if f.size == 0:
        return 0.0, (0, 0)
    at = np.unravel_index(np.argmax(f), f.shape)
    return float(f[at]), (int(at[0]), int(at[1]))


def score(case, Q, tile=64, forward_only_above=None):
    """Worst error / bar of the m x K result ``Q``: {"bw": backward, "fw": forward, "bw_at", "fw_at": (row, column)}; the
    rows outside the long-double sample enter "bw" with their float64 residual over TWO bars.  ``forward_only_above``:
    skip the long-double residual when the forward fraction alone already exceeds it (the fault tests)."""
    ref = reference(case, tile)
    Q = np.asarray(Q)
    assert Q.shape == (case.m, case.K) and Q.dtype == np.float64
    q = Q[ref.rows].astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        fw, fw_at = _fraction(np.abs(q - ref.q), ref.fw_bar)
        if forward_only_above is not None and fw > forward_only_above:
            return {"bw": 0.0, "fw": fw, "bw_at": (0, 0), "fw_at": (int(ref.rows[fw_at[0]]), fw_at[1])}
        bw, bw_at = _fraction(np.abs(q @ case.R.astype(LD) - ref.x), ref.bw_bar)
        bw_at = (int(ref.rows[bw_at[0]]), bw_at[1])
        if ref.rest.size:
            b2, at2 = _fraction(np.abs(Q[ref.rest] @ case.R - ref.rest_x), 2.0 * ref.rest_bar)
            if b2 > bw:
                bw, bw_at = b2, (int(ref.rest[at2[0]]), at2[1])
    return {"bw": bw, "fw": fw, "bw_at": bw_at, "fw_at": (int(ref.rows[fw_at[0]]), fw_at[1])}


# ---- float64 mirror of the two kernels -----------------------------------------------------------------------------------------

FAULTS = ("drop_last_update", "left_block_off", "col_ge_k_next_row", "store_ge_k_next_row", "ragged_row_stale",
          "zero_weight_multiplied", "weights_twice", "inplace_overwritten", "reciprocal_f32")


def fault_acts(fault, family, case):
    """Whether ``fault`` can move anything on this shape (see the module's docstring)."""
    K, m, k16 = case.K, case.m, k16_of(case.K)
    nbk = k16 // 16
    pw = 4 if family == FAMILY_13C else 8
    last_panel = nbk - (nbk - 1) // pw * pw
    tile = {FAMILY_13C: 64, FAMILY_13B16: 16, FAMILY_13B32: 32}[family]
    identity = np.array_equal(case.R, np.eye(K))          # K = 1 of illblock is R = [1]: a later pass leaves X as it is
    if fault == "drop_last_update":
        return last_panel >= 2
    if fault == "left_block_off":
        return nbk > pw
    if fault == "col_ge_k_next_row":
        # kernel 13B, packed rows, and a live row in front of a masked one (NaN / Inf)
        return (family != FAMILY_13C and case.first and case.lda == K and K < k16
                and bool(np.any(~case.dead[:-1] & case.dead[1:])))
    if fault == "store_ge_k_next_row":
        return K < k16 and bool(np.any(~case.dead[1:]))
    if fault == "ragged_row_stale":
        return m % tile != 0 and (case.first or not identity)
    if fault == "zero_weight_multiplied":
        return case.first and bool(case.dead.any())
    if fault == "weights_twice":
        return case.first and nbk > pw
    if fault == "inplace_overwritten":
        return not case.first and not identity
    if fault == "reciprocal_f32":
        rinv = 1.0 / np.diag(case.R)                                    # (K = 1 of illblock: R = [1])
        return family == FAMILY_13C and bool(np.any(rinv.astype(np.float32).astype(np.float64) != rinv))
    raise ValueError(fault)


def invert_diagonal_blocks(Rpad):
    """numpy port of fsnap::trsm_invert_diagonal_blocks: the float64 inverses of the 16 x 16 diagonal blocks."""
    nbk = Rpad.shape[0] // 16
    inv = np.zeros((nbk, 16, 16))
    for jb in range(nbk):
        T = Rpad[16 * jb:16 * jb + 16, 16 * jb:16 * jb + 16]
        X = inv[jb]
        for i in range(15, -1, -1):
            v = np.where(np.arange(16) == i, 1.0, 0.0)
            for k in range(i + 1, 16):
                v = v - T[i, k] * X[k]
            X[i, i:] = v[i:] / T[i, i]
    return inv


def mirror(case, family, fault=None):
    """The pass in float64 with the structure of ``family``'s kernel; returns Q (m x K).  A first pass starts from a
    buffer full of SENTINEL."""
    assert fault is None or fault in FAULTS
    m, K = case.m, case.K
    k16 = k16_of(K)
    nbk = k16 // 16
    c13 = family == FAMILY_13C
    pw = 4 if c13 else 8
    Rpad = np.eye(k16)
    Rpad[:K, :K] = np.triu(case.R)
    with np.errstate(invalid="ignore", over="ignore"):
        # the rows as the kernel loads them: K16 columns, the columns >= K of the last block selected to zero
        raw = np.zeros((m, k16))
        raw[:, :K] = case.A if case.first else case.X
        if fault == "col_ge_k_next_row" and K < k16:
            flat = np.concatenate([np.ascontiguousarray(raw[:, :K]).ravel(), np.zeros(k16)])
            for c in range(K, k16):
                raw[:, c] = flat[np.arange(m) * K + c]
        if case.first:
            wcol = case.weff[:, None]
            X = wcol * raw if fault == "zero_weight_multiplied" else np.where(case.dead[:, None], 0.0, wcol * raw)
        else:
            X = raw
        Q = np.zeros((m, k16))
        tinv = None if c13 else invert_diagonal_blocks(Rpad)

        def solve_block(x, jb):
            T = Rpad[16 * jb:16 * jb + 16, 16 * jb:16 * jb + 16]
            if c13:
                x = x.copy()
                rinv = 1.0 / np.diag(T)
                if fault == "reciprocal_f32":
                    rinv = rinv.astype(np.float32).astype(np.float64)
                for i in range(16):
                    x[:, i] = x[:, i] * rinv[i]
                    x[:, i + 1:] -= x[:, i:i + 1] * T[i:i + 1, i + 1:]
                return x
            q0 = x @ tinv[jb]
            r = x - q0 @ T
            return q0 + r @ tinv[jb]

        def run(X):
            for p0 in range(0, nbk, pw):
                blocks = range(p0, min(p0 + pw, nbk))
                cols = slice(16 * p0, 16 * blocks[-1] + 16)
                S = np.zeros((m, cols.stop - cols.start))
                for kb in range(p0):                                        # left-looking over the solved panels
                    qk = Q[:, 16 * kb:16 * kb + 16]
                    if fault == "weights_twice":
                        qk = case.weff[:, None] * qk
                    rb = kb + 1 if (fault == "left_block_off" and kb == p0 - 2) else kb
                    S += qk @ Rpad[16 * rb:16 * rb + 16, cols]
                for jb in blocks:                                           # right-looking inside the panel
                    o = 16 * (jb - p0)
                    q = solve_block(X[:, 16 * jb:16 * jb + 16] - S[:, o:o + 16], jb)
                    Q[:, 16 * jb:16 * jb + 16] = q
                    for lb in range(jb + 1, blocks[-1] + 1):
                        if fault == "drop_last_update" and lb == nbk - 1 and jb == nbk - 2:
                            continue
                        ol = 16 * (lb - p0)
                        S[:, ol:ol + 16] += q @ Rpad[16 * jb:16 * jb + 16, 16 * lb:16 * lb + 16]

        run(X)
        if fault == "inplace_overwritten":
            # the second block of the first panel (the only block when there is one) arrives solved already
            jb = 1 if nbk > 1 else 0
            X = X.copy()
            X[:, 16 * jb:16 * jb + 16] = Q[:, 16 * jb:16 * jb + 16]
            run(X)
        out = np.ascontiguousarray(Q[:, :K])
        if fault == "store_ge_k_next_row" and K < k16:
            flat = np.concatenate([out.ravel(), np.zeros(k16)])
            for c in range(K, k16):
                flat[np.arange(m) * K + c] = Q[:, c]
            out = flat[:m * K].reshape(m, K)
        if fault == "ragged_row_stale":
            out[m - 1] = SENTINEL if case.first else case.X[m - 1]
    return out
