"""GPU (-m gpu): the row-streaming kernels of fsnap_rows.hip -- kernel 3 (weight_rows), kernel 4 (gemv_rows: predictions,
weighted SSE, u), kernel 7 (gemvT_rows + colsum_partials), kernel 4+7 (residual_rows<NJ>) and kernel 9 (error_stats) --
through _capi.HipContext, against the long-double references of tests/rows_cases.py under its a-priori bars (their
derivation: the docstring there; that they are neither loose nor wrong: tests/test_rows_cases_cpu.py).

Every test prints one line per case with the worst error / bar of each output: aw, bw (0 = the bits of the float64
product), p, sse (of fsnap_predict), then s and sse of fsnap_residual_rhs in the one-pass form (s1, sse1; K <= 288) and in
the two-kernel form (s0, sse0).  Everything is asserted at <= 1.0 bars."""
import types

import numpy as np
import pytest

from fitsnap_amd import _capi

import rows_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _capi.HipContext(0)
    yield c
    c.close()


def mask_u8(case):
    return None if case.mask is None else case.mask.astype(np.uint8)


def run_kernels(ctx, case, forms=None):
    """weight_rows, predict and residual_rhs (fused_residual = 1 where K allows it, and 0) on the rows now on ``ctx``."""
    forms = ((1, 0) if case.K <= rc.FUSED_MAX_K else (0,)) if forms is None else forms
    out = {}
    out["aw"], out["bw"] = ctx.weight_rows()
    out["p"], out["sse"] = ctx.predict(case.beta, want_preds=True, want_sse=True)
    try:
        for mode in forms:
            ctx.set_option("fused_residual", mode)
            out[f"s{mode}"], out[f"sse{mode}"] = ctx.residual_rhs(case.beta, want_sse=True)
    finally:
        ctx.set_option("fused_residual", 1)
    return out


def run_case(ctx, case, forms=None):
    ctx.upload_rows(np.ascontiguousarray(case.A), case.b)
    ctx.set_weights(case.w, mask_u8(case))
    return run_kernels(ctx, case, forms)


def check(case, out, rows=None, tag=""):
    """All outputs within their bars (the predictions of ``rows`` only, when given); prints the line of the case."""
    res = rc.score(case, {k: out[k] for k in ("aw", "bw", "p", "sse") if k in out}, rows=rows)
    ref = rc.reference(case)
    for mode in (1, 0):
        if f"s{mode}" in out:
            got = rc.score(case, {"s": out[f"s{mode}"], "sse": out[f"sse{mode}"]})
            res[f"s{mode}"], res[f"sse{mode}"] = got["s"], got["sse"]
    if "s1" in out and "s0" in out:
        res["s1-s0"] = rc.worst(out["s1"], out["s0"], ref.s_bar)
    print(f"{tag}{case.name}: " + " ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, res
    return res


def same_outputs(x, y, keys=None):
    keys = [k for k in x if k in y] if keys is None else keys
    bad = [k for k in keys if not rc.same_bits(np.atleast_1d(x[k]), np.atleast_1d(y[k]))]
    assert not bad, bad


# ---- geometry ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", rc.K_SWEEP)
def test_k_sweep(ctx, K):
    """Both sides of every switch of the launchers (lane widths of kernels 3 and 7, their second column pass, NJ of kernel
    4+7, its end at 288, 16-byte loads of odd-width rows); K <= 288 runs both residual forms and they agree under the bar."""
    case = rc.make_case(rc.sweep_m(K), K)
    out = run_case(ctx, case)
    assert ("s1" in out) == (K <= rc.FUSED_MAX_K) and "s0" in out
    check(case, out)


@pytest.mark.parametrize("K", rc.M_SWEEP_K)
def test_m_sweep(ctx, K):
    """Tiny and ragged row counts: fewer rows than a wave's group, than a workgroup's rows, one more than a multiple."""
    for m in rc.M_SWEEP:
        case = rc.make_case(m, K)
        check(case, run_case(ctx, case))


@pytest.mark.parametrize("m,K", rc.GRID_CASES)
def test_grid_caps(ctx, m, K):
    """Below, at and beyond the grid caps: the grid-stride loops of kernels 4 and 4+7 (65536 rows at NJ = 1, 16384 at
    NJ = 9) and the workgroups of kernel 7 whose row range is empty (m = 131073: rows_per_wg = 65)."""
    case = rc.make_case(m, K)
    check(case, run_case(ctx, case))


# ---- layouts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,lda", rc.LAYOUT_CASES)
def test_padded_rows_in_caller_owned_memory(K, lda):
    """lda = K + 5 and lda = K + 1 with NaN in the padding columns: rows, weights and mask bound in caller-owned device
    memory (bind_rows / bind_weights), and the same strided rows through upload_rows.  Within the bars, and every output
    has the bits of the contiguous upload (no kernel's summation order depends on the leading dimension)."""
    import torch

    case = rc.make_case(rc.LAYOUT_M, K, lda)
    assert case.A.strides[0] == 8 * lda and np.isnan(case.big[:, K:]).all()
    dev = torch.device("cuda", 0)
    dbig, db, dw = (torch.from_numpy(np.array(a)).to(dev) for a in (case.big, case.b, case.w))
    dm = torch.from_numpy(mask_u8(case)).to(dev)
    torch.cuda.synchronize()
    c = _capi.HipContext(0)
    try:
        c.bind_rows(dbig.data_ptr(), case.m, K, lda, db.data_ptr())
        c.bind_weights(dw.data_ptr(), dm.data_ptr())
        bound = run_kernels(c, case)
        check(case, bound, tag="bound ")
        c.upload_rows(case.A, case.b)                       # the strided host view: padding stays behind
        c.set_weights(case.w, mask_u8(case))
        strided = run_kernels(c, case)
        dense = run_case(c, case)
        check(case, dense, tag="dense ")
        same_outputs(bound, dense)
        same_outputs(strided, dense)
    finally:
        torch.cuda.synchronize()
        c.close()


@pytest.mark.parametrize("K", [31, 300])
def test_no_mask_at_all(ctx, K):
    """set_weights without a mask: the kernels run on the context's all-ones mask."""
    case = rc.make_case(rc.LAYOUT_M, K, None, False)
    check(case, run_case(ctx, case))


# ---- garbage in masked rows ---------------------------------------------------------------------------------------------------

def garbage_stats_case(case):
    """Five categories over the training rows of ``case``, -1 on its test rows."""
    cat = np.where(case.mask, np.arange(case.m) % 5, -1).astype(np.int32)
    return types.SimpleNamespace(name=case.name + " ncat=5", m=case.m, K=case.K, ncat=5, A=case.A, b=case.b, w=case.w,
                                 beta=case.beta, cat=cat)


@pytest.mark.parametrize("K", rc.GARBAGE_K)
def test_masked_rows_may_hold_garbage(ctx, K):
    """NaN in A, Inf in b and -Inf in w of the test rows reach nothing: the reference drops those rows by fancy indexing
    (svd.py:44-46), and the SYRK is held to the same (test_tiled_kernel_masked_rows_may_hold_garbage).  sse and s of both
    residual forms stay finite, within the bar and bit-identical to the run on the clean rows -- which, for the two-kernel
    form, also says that kernel 7 gives finite rows the bits it gave before it learnt to skip rows with u = 0; aw, bw of
    masked rows are +0.0; predictions of training rows keep their bits; the error statistics skip rows of no category."""
    case = rc.make_case(rc.GARBAGE_M, K)
    train = case.mask
    clean = run_case(ctx, case)
    check(case, clean, tag="clean ")
    sc = garbage_stats_case(case)
    big, b, w = rc.with_garbage(case)
    ctx.upload_rows(big, b)
    ctx.set_weights(w, mask_u8(case))
    dirty = run_kernels(ctx, case)
    stats = ctx.error_stats(case.beta, sc.cat, sc.ncat)
    for k in ("sse", "s1", "sse1", "s0", "sse0"):
        if k in dirty:
            assert np.all(np.isfinite(dirty[k])), k
    check(case, dirty, rows=train, tag="dirty ")
    same_outputs(clean, dirty, [k for k in dirty if k not in ("p", "aw", "bw")])
    assert rc.same_bits(dirty["p"][train], clean["p"][train]) and np.isnan(dirty["p"][~train]).all()
    zero = np.zeros(1).view(np.int64)[0]
    assert np.all(dirty["aw"][~train].view(np.int64) == zero) and np.all(dirty["bw"][~train].view(np.int64) == zero)
    assert rc.same_bits(dirty["aw"], clean["aw"]) and rc.same_bits(dirty["bw"], clean["bw"])
    cols = rc.stats_score(sc, stats)
    print(f"dirty {sc.name}: stats " + " ".join(f"{v:.3g}" for v in cols))
    assert np.isfinite(stats).all() and max(cols) <= 1.0, cols


# ---- row independence and determinism -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [7, 31, 129, 289])
def test_rows_are_independent_and_runs_repeat(ctx, K):
    """A row's prediction and weighted row keep their bits under a row permutation and under truncation of m (an odd-width
    row's 16-byte load must not let its neighbour's first element in); weight_rows, predict and residual_rhs are
    bit-identical on repeat."""
    case = rc.make_case(rc.LAYOUT_M, K)
    first = run_case(ctx, case)
    check(case, first)
    same_outputs(first, run_kernels(ctx, case))
    perm = np.random.default_rng(K).permutation(case.m)
    A, w, mk = np.ascontiguousarray(case.A), case.w, mask_u8(case)
    ctx.upload_rows(A[perm], case.b[perm])
    ctx.set_weights(w[perm], mk[perm])
    aw, bw = ctx.weight_rows()
    p, _ = ctx.predict(case.beta)
    assert rc.same_bits(p, first["p"][perm]) and rc.same_bits(aw, first["aw"][perm]) and rc.same_bits(bw, first["bw"][perm])
    for cut in (case.m - 1, case.m - 37, 130):
        ctx.upload_rows(A[:cut], case.b[:cut])
        ctx.set_weights(w[:cut], mk[:cut])
        aw, bw = ctx.weight_rows()
        p, _ = ctx.predict(case.beta)
        assert rc.same_bits(p, first["p"][:cut]) and rc.same_bits(aw, first["aw"][:cut]) and rc.same_bits(bw, first["bw"][:cut])


# ---- error statistics ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,K,ncat", rc.STATS_CASES)
def test_error_stats(ctx, m, K, ncat):
    """Kernel 9 at 1, 37 and 3000 categories (the limit of its LDS table) and in its grid-stride loop (m > 512 x 4096):
    exact counts, every sum within its any-order bar; an empty category is all zero, a one-row category has no spread, a
    category whose weights are all zero has n_w = 0 and zero weighted columns; ids of -1 and >= ncat are ignored."""
    case = rc.make_stats_case(m, K, ncat)
    ref, _, _ = rc.stats_reference(case)
    ctx.upload_rows(case.A, case.b)
    ctx.set_weights(case.w)
    st = ctx.error_stats(case.beta, case.cat, ncat)
    cols = rc.stats_score(case, st)
    print(f"{case.name}: stats " + " ".join(f"{v:.3g}" for v in cols))
    assert st.shape == (ncat, 10) and max(cols) <= 1.0, cols
    assert np.array_equal(st[:, :2], ref[:, :2].astype(np.float64))
    if ncat >= 4:
        assert not st[case.empty].any()
        assert st[case.single, 0] == 1 and st[case.single, 6] == 0 and st[case.single, 9] == 0 and st[case.single, 2] == case.b[case.cat == case.single][0]
        assert st[case.zero_w, 0] >= 2 and st[case.zero_w, 1] == 0 and not st[case.zero_w, [3, 7, 8, 9]].any()
        assert st[case.zero_w, 6] > 0


def test_error_stats_refuses_more_categories_than_its_table_holds(ctx):
    case = rc.make_stats_case(*rc.STATS_CASES[0])
    ctx.upload_rows(case.A, case.b)
    ctx.set_weights(case.w)
    ncat = rc.STATS_MAX_NCAT + 1
    cat = np.zeros(case.m, dtype=np.int32)
    st = np.empty((ncat, 10))
    rc_ = ctx._lib.fsnap_error_stats(ctx._h, _capi._ptr(case.beta), _capi._ptr(cat), ncat, _capi._ptr(st))
    assert rc_ == _capi.E_ARG
    with pytest.raises(ValueError, match="3000"):
        ctx.error_stats(case.beta, cat, ncat)
    assert ctx.error_stats(case.beta, cat, rc.STATS_MAX_NCAT)[0, 0] == case.m      # the limit itself runs
