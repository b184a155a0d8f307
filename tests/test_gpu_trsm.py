"""GPU (-m gpu): ONE pass Q <- X R^-1 of the row-space solve -- kernel 13C ``fsnap_trsm_acc2_k<NB, FIRST>`` and kernel 13B
``fsnap_trsm_panel_k<TR, KG, FIRST>`` of fsnap_trsm.hip -- through ``HipContext.trsm_pass`` with the family named, against
the long-double reference of tests/trsm_cases.py under its a-priori backward and forward bars (their derivation: the
docstring there; that they are neither loose nor wrong: tests/test_trsm_cases_cpu.py).

Every case runs inside an allocation with 64 guard rows of a sentinel in front of and behind Q and asserts that the guards
come back bit for bit, that the rows of zero effective weight are +0.0 bit for bit, and both bars at <= 1.0 on every row
(beyond m K^2 = 1e8: on the sampled rows, the others at two bars of the float64 residual).  One line per case with the worst
error / bar and where; the module's last lines list the worst case per (family, first, kind): the table of
profiles/trsm_accuracy.txt."""
import numpy as np
import pytest

from fitsnap_amd import _capi

import trsm_cases as tc

pytestmark = pytest.mark.gpu

F13C, F16, F32 = tc.FAMILY_13C, tc.FAMILY_13B16, tc.FAMILY_13B32
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    c = _capi.HipContext(0)
    yield c
    c.close()
    print("\nworst error / bar per (family, first, kind): backward at (m, K, row, column) | forward at ... | largest cond(T)")
    for key in sorted(WORST):
        w = WORST[key]
        print(f"  family {key[0]} {'first' if key[1] else 'later'} {key[2]:8s} bw {w['bw'][0]:.3f} at {w['bw'][1]} | "
              f"fw {w['fw'][0]:.3f} at {w['fw'][1]} | cond(T) {w['cond']:.2g} | {w['n']} cases")


def load(ctx, case):
    """The rows of a first pass (with their NaN / Inf), or -- a later pass needs the shape only -- its finite X."""
    ctx.upload_rows(np.ascontiguousarray(case.A if case.first else case.X), case.b)
    ctx.set_weights(case.w, case.mask.astype(np.uint8))


def run_pass(ctx, case, family, X=None, R=None):
    """One pass on the rows now on ``ctx``: Q (m x K) out of an allocation with guard rows, which must come back intact."""
    import torch

    m, K, g = case.m, case.K, tc.GUARD_ROWS
    host = np.full((m + 2 * g, K), tc.SENTINEL)
    if not case.first:
        host[g:g + m] = case.X if X is None else X
    buf = torch.from_numpy(host).to(torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    ran = ctx.trsm_pass(case.R if R is None else R, case.first, buf.data_ptr() + g * K * 8, family)
    assert ran == (family or tc.rule(m, K)), f"{case.name}: family {ran} ran, not {family or tc.rule(m, K)}"
    out = buf.cpu().numpy()
    sentinel = np.full((g, K), tc.SENTINEL)
    assert tc.same_bits(out[:g], sentinel) and tc.same_bits(out[g + m:], sentinel), f"{case.name}: guard rows overwritten"
    return np.ascontiguousarray(out[g:g + m])


def check(case, family, Q, tag=""):
    """Zero rows are +0.0 bit for bit, every other row is finite and within both bars; records the worst of its kind."""
    res = tc.score(case, Q)
    print(f"{tag}{case.name} family {family} [{tc.instance(family, case.first, case.K)}]: bw {res['bw']:.3f} at {res['bw_at']} "
          f"fw {res['fw']:.3f} at {res['fw_at']}")
    assert not Q[case.dead].view(np.int64).any(), f"{case.name}: a row of zero weight is not +0.0"
    assert np.isfinite(Q).all(), f"{case.name}: NaN / Inf reached a live row"
    assert res["bw"] <= 1.0 and res["fw"] <= 1.0, (case.name, family, res)
    w = WORST.setdefault((family, case.first, case.kind), {"bw": (0.0, None), "fw": (0.0, None), "cond": 0.0, "n": 0})
    for k in ("bw", "fw"):
        if res[k] >= w[k][0]:
            w[k] = (res[k], (case.m, case.K) + res[k + "_at"])
    w["cond"], w["n"] = max(w["cond"], case.fac.cond_t), w["n"] + 1
    return res


def sweep(ctx, family, K, cases):
    for first, kind, m in cases:
        case = tc.make_case(m, K, kind, first)
        load(ctx, case)
        check(case, family, run_pass(ctx, case, family))


# ---- geometry ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", tc.C_COLS)
def test_13c_column_sweep(ctx, K):
    """Every NB = 1 ... 9 (129 ... 144 columns with the family forced: production runs them from 32 768 rows on), both panel
    boundaries, a last block of 1 ... 16 columns; three unguarded 64-row tiles + a ragged one; both passes, all factors."""
    sweep(ctx, F13C, K, [(first, kind, tc.C_COLS_M) for first in (True, False) for kind in tc.KINDS])


@pytest.mark.parametrize("K", tc.C_ROWS_K)
def test_13c_row_sweep(ctx, K):
    """Fewer rows than a tile, one tile, one row more; K = 142 is NB = 9."""
    sweep(ctx, F13C, K, [(first, kind, m) for first in (True, False) for m in tc.C_ROWS_M for kind in ("benign", "cholqr")])


B_COL_PARAMS = [(fam, K, kind, first) for K in tc.B_COLS for kind in tc.b_kinds(K) for fam in (F16, F32)
                for first in ((None,) if K < 1024 else (True, False))]


@pytest.mark.parametrize("fam,K,kind,first", B_COL_PARAMS)
def test_13b_column_sweep(ctx, fam, K, kind, first):
    """16- and 32-row tiles at K = K16 and K16 - 15 for every K16 = 144 ... 400, and 512, 513, 1024, 1595: a last panel of
    1 ... 8 blocks with 2, 3 and 4 panels, last panels shorter than a slab of R, 13 panels; two full workgroups + 37 rows."""
    sweep(ctx, fam, K, [(f, kind, tc.B_COLS_M[fam]) for f in ((True, False) if first is None else (first,))])


@pytest.mark.parametrize("fam", [F16, F32])
@pytest.mark.parametrize("K", tc.B_ROWS_K)
def test_13b_row_sweep(ctx, fam, K):
    """Fewer rows than a wave's tile, than a workgroup, one more; waves and workgroups without rows."""
    sweep(ctx, fam, K, [(first, kind, m) for first in (True, False) for m in tc.B_ROWS_M for kind in ("benign", "cholqr")])


# ---- layout ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", tc.LAYOUT_K)
def test_first_pass_from_padded_rows_in_caller_owned_memory(K):
    """lda = K + 1, K + 5 and K rounded up to 16, NaN in the padding columns, rows / weights / mask bound in caller-owned
    device memory: within the bars and bit-identical to the first pass from the packed copy, per family."""
    import torch

    dev = torch.device("cuda", 0)
    fams = [f for f in (F13C, F16, F32) if tc.family_runs(f, K)]
    packed = tc.make_case(tc.LAYOUT_M, K, "benign", True)
    c = _capi.HipContext(0)
    try:
        load(c, packed)
        want = {f: run_pass(c, packed, f) for f in fams}
        for f in fams:
            check(packed, f, want[f], tag="packed ")
        for lda in sorted({K + 1, K + 5, tc.k16_of(K)} - {K}):
            case = tc.make_case(tc.LAYOUT_M, K, "benign", True, lda)
            assert case.big.shape[1] == lda and np.isnan(case.big[:, K:]).all() and tc.same_bits(case.w, packed.w)
            live = ~case.dead
            assert tc.same_bits(case.A[live], packed.A[live]) and np.array_equal(case.dead, packed.dead)
            dbig, db, dw = (torch.from_numpy(np.array(a)).to(dev) for a in (case.big, case.b, case.w))
            dm = torch.from_numpy(case.mask.astype(np.uint8)).to(dev)
            torch.cuda.synchronize()
            c.bind_rows(dbig.data_ptr(), case.m, K, lda, db.data_ptr())
            c.bind_weights(dw.data_ptr(), dm.data_ptr())
            for f in fams:
                Q = run_pass(c, case, f)
                check(case, f, Q, tag="bound ")
                assert tc.same_bits(Q, want[f]), (K, lda, f)
            torch.cuda.synchronize()
    finally:
        c.close()


# ---- exactness -----------------------------------------------------------------------------------------------------------------

EXACT = [(F13C, 31), (F13C, 113), (F13C, 142), (F16, 145), (F32, 145), (F16, 300), (F32, 300)]


@pytest.mark.parametrize("fam,K", EXACT)
@pytest.mark.parametrize("first", [True, False])
def test_runs_repeat_and_a_row_does_not_depend_on_its_place(ctx, fam, K, first):
    """Two runs are bit-identical; the same rows in reversed order give the reversed Q bit for bit (a row's arithmetic does
    not depend on its place in a tile, its wave or its workgroup); NaN / Inf of the rows of zero weight reach no other row
    and those rows are +0.0 (``check``)."""
    case = tc.make_case(293, K, "benign", first)
    load(ctx, case)
    Q = run_pass(ctx, case, fam)
    check(case, fam, Q)
    assert tc.same_bits(run_pass(ctx, case, fam), Q)
    rev = slice(None, None, -1)
    ctx.upload_rows(np.ascontiguousarray((case.A if first else case.X)[rev]), case.b[rev])
    ctx.set_weights(np.ascontiguousarray(case.w[rev]), np.ascontiguousarray(case.mask[rev]).astype(np.uint8))
    Qr = run_pass(ctx, case, fam, X=None if first else np.ascontiguousarray(case.X[rev]))
    assert tc.same_bits(Qr, np.ascontiguousarray(Q[rev]))


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1003])
def test_qpack_pairs_are_exact(ctx, m):
    """fsnap_qpack_k: (w_eff != 0, w_eff b) per row, exactly; nothing behind row m."""
    import torch

    case = tc.make_case(m, 17, "benign", True)
    load(ctx, case)
    buf = torch.full((2 * m + 64,), tc.SENTINEL, dtype=torch.float64, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    ctx.qpack_device(buf.data_ptr())
    out = buf.cpu().numpy()
    want = np.stack([(case.weff != 0).astype(np.float64), np.where(case.weff != 0, case.weff * case.b, 0.0)], axis=1)
    assert tc.same_bits(out[:2 * m].reshape(m, 2), want) and tc.same_bits(out[2 * m:], np.full(64, tc.SENTINEL))


# ---- dispatch ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,K,fam", tc.DISPATCH)
def test_family_zero_is_the_family_the_rule_names(ctx, m, K, fam):
    """family = 0 at both sides of the rule's switches (32 768 rows at K16 = 144 and beyond it, K16 = 128) equals the named
    family bit for bit, in both passes -- the only large shapes of the module.  The two forms of kernel 13B give a row the
    same bits (its arithmetic depends on neither TR nor KG), so the bits pin the 13C / 13B switch only; the switch between
    the 16- and the 32-row tiles is pinned by the family that fsnap_trsm_pass reports to have run (``run_pass`` asserts it
    on every call: with family = 0 it is the rule's own answer, the function fsnap_lstsq_rows launches through)."""
    assert tc.rule(m, K) == fam
    for first in (True, False):
        case = tc.make_case(m, K, "benign", first)
        load(ctx, case)
        Q = run_pass(ctx, case, fam)
        check(case, fam, Q)
        assert tc.same_bits(run_pass(ctx, case, 0), Q)


def test_a_family_outside_its_widths_is_an_argument_error(ctx):
    import torch

    fresh = _capi.HipContext(0)
    try:
        buf = torch.zeros(8, dtype=torch.float64, device=torch.device("cuda", 0))
        with pytest.raises(_capi.FsnapError, match="no rows"):
            fresh.qpack_device(buf.data_ptr())
    finally:
        fresh.close()

    for K, bad in ((128, (F16, F32)), (145, (F13C,))):
        case = tc.make_case(65, K, "benign", False)
        load(ctx, case)
        buf = torch.zeros((65, K), dtype=torch.float64, device=torch.device("cuda", ctx.device))
        torch.cuda.synchronize()
        for f in bad + (4, -1):
            rc_ = ctx._lib.fsnap_trsm_pass(ctx._h, _capi._ptr(case.R), 0, f, _capi.c_void_p(buf.data_ptr()), None)
            assert rc_ == _capi.E_ARG, (K, f)
            with pytest.raises(ValueError):
                ctx.trsm_pass(case.R, False, buf.data_ptr(), f)
        assert not buf.cpu().numpy().any()


# ---- the call the solver makes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,K", [(5003, 113), (3001, 208)])
def test_first_pass_of_lstsq_rows_replayed(m, K):
    """lstsq_rows on graded rows of kappa 1e6 (one 13C width, one 13B width; NaN in the masked rows), then the same rows
    through the host step of its first pass (rowspace_factor on the statistics the context computes) and one pass of the
    entry tested above with the kernel the solver picks: the factor the solver really forms meets the bars."""
    base = tc.make_case(m, K, "cholqr", True)
    A = np.array(base.A)
    A[base.dead] = 1.0                                   # rows of zero weight inside the training set: finite
    A[~base.mask] = np.nan
    c = _capi.HipContext(0)
    try:
        c.upload_rows(A, base.b)
        c.set_weights(base.w, base.mask.astype(np.uint8))
        beta, rank, info = c.lstsq_rows(1.0e-13)
        assert np.isfinite(beta).all() and info["passes"] >= 1
        G, _, _ = c.normal_eq()
        Rp, _, _ = _capi.rowspace_factor(G)
        assert Rp is not None and not np.tril(Rp, -1).any()
        case = tc.first_pass_case(A, base.b, base.w, base.mask, Rp, f"solver factor {m}x{K}")
        fam = tc.rule(m, K)
        Q = run_pass(c, case, 0)
        check(case, fam, Q, tag="replay ")
        assert tc.same_bits(run_pass(c, case, fam), Q)
        print(f"    max |Q^T Q - I| after the first pass {np.max(np.abs(Q.T @ Q - np.eye(K))):.2e}, lstsq_rows: "
              f"{info['passes']:.0f} passes, rank {rank}")
    finally:
        c.close()
