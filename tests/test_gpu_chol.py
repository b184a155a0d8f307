"""GPU (-m gpu): the blocked device Cholesky chain of fsnap_chol.hip -- scaling + first diagonal block, one fused launch per
64-row panel, the macro-blocked back substitution, the forward sweep for further right-hand sides (8f), the probe Gram and
the factor-only form -- against the long-double reference of tests/chol_cases.py under its a-priori bars (derivation: the
docstring there; that they are neither loose nor wrong: tests/test_chol_cases_cpu.py).

The statistics are uploaded as they are ([G | c | 3 scalars], no rows, no SYRK), so the chain sees matrices the rows of a test
never produce: 3 to 13 panels with every panel count modulo 4 (top macro-blocks of 1, 2, 3 and 4 panels), pivots down to
2.5e-3 next to the acceptance threshold 1e-3, column scales over 6 and 16 decades, hidden conditioning.

Every solve prints one line ``chol <case> <kind> panels P top T: bwd .. fwd .. est ..`` with the worst error / bar of each
check; everything is asserted at <= 1.0 bars."""
import contextlib

import numpy as np
import pytest

from fitsnap_amd import _capi
from oracle import fitsnap_oracle as orc

import chol_cases as cc

pytestmark = pytest.mark.gpu
EPS = cc.EPS
RCOND = 1.0e-13
KIND_NAMES = {_capi.SOLVE_CHOL: "CHOL", _capi.SOLVE_LSTSQ: "LSTSQ", _capi.SOLVE_RIDGE: "RIDGE", _capi.SOLVE_LSTSQ_PROBE: "LSTSQ_PROBE"}
LSTSQ_KINDS = (_capi.SOLVE_LSTSQ, _capi.SOLVE_LSTSQ_PROBE)


class Buffer:
    """One caller-owned device buffer for the packed statistics, grown on demand (caller-owned: every solve factorises)."""

    def __init__(self, ctx):
        self.ctx, self.ptr, self.cap = ctx, None, 0

    def load(self, G, c):
        p = cc.packed(G, c)
        if p.nbytes > self.cap:
            self.free()
            self.ptr, self.cap = self.ctx.dev_alloc(p.nbytes), p.nbytes
        self.ctx.dev_upload(self.ptr, p)
        return self.ptr

    def free(self):
        if self.ptr is not None:
            self.ctx.dev_free(self.ptr)
        self.ptr, self.cap = None, 0


@pytest.fixture(scope="module")
def ctx():
    c = _capi.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def buf(ctx):
    b = Buffer(ctx)
    yield b
    b.free()


@contextlib.contextmanager
def on_device(ctx, K):
    """Below fsnap::DEVICE_CHOL_MIN_K the device factorises only with device_solve = 1."""
    if K < cc.DEVICE_MIN_K:
        ctx.set_option("device_solve", 1)
    try:
        yield
    finally:
        ctx.set_option("device_solve", 0)


def param_of(kind, ref):
    return RCOND if kind in LSTSQ_KINDS else (ref.alpha if kind == _capi.SOLVE_RIDGE else 0.0)


def report(ref, kind, res, extra=""):
    print(f"chol {ref.name} {KIND_NAMES.get(kind, kind)} panels {cc.panels(ref.K)} top {cc.top_block(ref.K)}{extra}: "
          + " ".join(f"{k} {v:.3g}" for k, v in res.items()))


def device_solve(ctx, ptr, ref, kind, tag=""):
    """One factorising solve of the statistics at ``ptr``: answered by the device, within the bars; returns (beta, rcond)."""
    K = ref.K
    beta, rank, rcond = ctx.solve_device(kind, param_of(kind, ref), K, ptr)
    piv, est, steps, where = _capi.cond_info()
    lstsq = kind in LSTSQ_KINDS
    res = cc.score(ref, beta, est if lstsq else None)
    report(ref, kind, res, f"{tag} pivot {piv:.3g}")
    assert rank == K and where == 1, (rank, where)                 # the device answered, not the host fallback
    assert piv > cc.ACCEPT_PIVOT
    assert max(res.values()) <= 1.0, res
    if lstsq:
        assert steps == 1 and cc.in_band(ref, est), (steps, est, ref.lam_min)
        assert rcond == min(piv, est)
    else:
        assert steps == 0
    return beta, rcond


# ---- 1. geometry sweep on uploaded statistics -----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", cc.K_SWEEP)
def test_geometry_sweep(ctx, buf, K):
    """3 to 13 panels, every panel count modulo 4, K modulo 64 in {0, 1, 17, 63, ...}: a well-conditioned family and one next
    to the acceptance threshold, as a ridge solve with alpha = 0 and as LSTSQ (which adds the probe Gram and the estimate)."""
    with on_device(ctx, K):
        for name in cc.SWEEP_FAMILIES:
            ref = cc.reference(name, K)
            ptr = buf.load(ref.G, ref.c)
            for kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_LSTSQ):
                device_solve(ctx, ptr, ref, kind)


@pytest.mark.parametrize("K", cc.K_MOD4)
def test_other_families_kinds_and_ridge_terms(ctx, buf, K):
    """One K per panel count modulo 4: the remaining families, SOLVE_CHOL and SOLVE_LSTSQ_PROBE, and ridge terms at both ends
    (1e-8 and 1e12 times the largest diagonal entry: at the upper end H is the identity to rounding)."""
    for name in cc.OTHER_FAMILIES:
        ref = cc.reference(name, K)
        ptr = buf.load(ref.G, ref.c)
        for kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_LSTSQ):
            device_solve(ctx, ptr, ref, kind)
    for name in cc.SWEEP_FAMILIES:
        ref = cc.reference(name, K)
        ptr = buf.load(ref.G, ref.c)
        for kind in (_capi.SOLVE_CHOL, _capi.SOLVE_LSTSQ_PROBE):
            device_solve(ctx, ptr, ref, kind)
    for alpha_rel in cc.ALPHAS:
        ref = cc.reference("gauss", K, alpha_rel)
        ptr = buf.load(ref.G, ref.c)
        device_solve(ctx, ptr, ref, _capi.SOLVE_RIDGE)


@pytest.mark.parametrize("K", cc.K_LARGE)
def test_large_widths(ctx, buf, K):
    ref = cc.reference("gauss", K)
    ptr = buf.load(ref.G, ref.c)
    for kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_LSTSQ):
        device_solve(ctx, ptr, ref, kind)


# ---- 2. / 3. further right-hand sides on the factor (8f + 8e), bits -------------------------------------------------------------

def resident_buffer(ctx, K):
    """The context's OWN statistics buffer at width K (the only one whose factor is kept for further right-hand sides)."""
    r = np.random.default_rng(K)
    ctx.upload_rows(r.standard_normal((8, K)), r.standard_normal(8))
    ctx.set_weights(np.ones(8))
    return ctx.normal_eq_resident()


@pytest.mark.parametrize("K", cc.K_RHS)
@pytest.mark.parametrize("name", cc.SWEEP_FAMILIES)
def test_further_right_hand_sides_reuse_the_factor(ctx, name, K):
    ref = cc.reference(name, K)
    r = np.random.default_rng(K + 1)
    with on_device(ctx, K):
        ptr = resident_buffer(ctx, K)
        ctx.dev_upload(ptr, cc.packed(ref.G, ref.c))              # clears the factor tag, as an in-place all-reduce would
        _, rcond = device_solve(ctx, ptr, ref, _capi.SOLVE_LSTSQ, " (own buffer)")
        for c2 in (r.standard_normal(K) / ref.d, ref.G @ (r.standard_normal(K) * ref.d)):
            beta, rank, rc2 = ctx.solve_device(_capi.SOLVE_LSTSQ, RCOND, K, ptr, rhs=c2)
            piv, est, steps, where = _capi.cond_info()
            res = cc.score(ref, beta, c=c2, rhs_ref=cc.reference_rhs(ref, c2))
            report(ref, _capi.SOLVE_LSTSQ, res, " rhs")
            assert rank == K and where == 1 and steps == 0         # two sweeps with the factor: no factorisation, no estimate
            assert rc2 == rcond
            assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("K", cc.K_RHS)
def test_solves_are_bit_identical_from_run_to_run(ctx, K):
    """The hand-offs inside the diagonal pipeline are polled and unordered; a race there shows first as bits that change."""
    fam = cc.family("spectrum3e4", K)
    p = cc.packed(fam.G, fam.c)
    c2 = np.random.default_rng(K + 2).standard_normal(K) / np.sqrt(np.diag(fam.G))
    with on_device(ctx, K):
        ptr = resident_buffer(ctx, K)
        first = again = None
        for _ in range(3):
            ctx.dev_upload(ptr, p)
            beta, rank, rcond = ctx.solve_device(_capi.SOLVE_LSTSQ, RCOND, K, ptr)
            info = _capi.cond_info()
            assert rank == K and info[2:] == (1, 1)
            if first is None:
                first = (beta, rcond, info)
            assert cc.same_bits(beta, first[0]) and rcond == first[1] and info == first[2]
        for _ in range(3):
            beta, rank, rcond = ctx.solve_device(_capi.SOLVE_LSTSQ, RCOND, K, ptr, rhs=c2)
            assert rank == K and _capi.cond_info()[2:] == (0, 1)
            if again is None:
                again = beta
            assert cc.same_bits(beta, again) and rcond == first[1]
    print(f"chol spectrum3e4-K{K} bits: 3 factorising + 3 reuse solves identical")


# ---- 4. acceptance edge and status hygiene --------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (257, 448))
def test_refused_systems_come_back_through_the_host_path(ctx, buf, K):
    ref = cc.reference("spectrum1e6", K)                            # pivot 1.5e-4: below the threshold, far above 64 K eps
    ptr = buf.load(ref.G, ref.c)
    for kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_LSTSQ):
        beta, rank, _ = ctx.solve_device(kind, param_of(kind, ref), K, ptr)
        piv, est, steps, where = _capi.cond_info()
        res = {"fwd": cc.forward(ref, beta)}
        report(ref, kind, res, " host path")
        assert rank == K and where == 0
        assert res["fwd"] <= 1.0, res
    # a duplicated column: what test_large_k_device_cholesky_falls_back_when_ill_conditioned asserts
    dup = cc.family("dup", K)
    ptr = buf.load(dup.G, dup.c)
    beta, rank, _ = ctx.solve_device(_capi.SOLVE_LSTSQ, RCOND, K, ptr)
    assert _capi.cond_info()[3] == 0
    with pytest.raises(np.linalg.LinAlgError):
        ctx.solve_device(_capi.SOLVE_CHOL, 0.0, K, ptr)
    assert rank == K - 1
    want = np.linalg.lstsq(dup.rows, dup.y, rcond=RCOND)[0]
    assert np.max(np.abs(dup.rows @ beta - dup.rows @ want)) < 1e-8 * np.max(np.abs(dup.y))


def outcome(call):
    try:
        beta, rank, rcond = call()
    except Exception as e:                                          # noqa: BLE001 -- the type of the error is the outcome
        return (type(e).__name__,)
    return ("ok", rank, beta, rcond)


@pytest.mark.parametrize("what", ["nan_diagonal", "zero_column"])
def test_unusable_diagonal_behaves_as_the_host_solver(ctx, buf, what):
    K = 257
    fam = cc.family("gauss", K)
    G, c = fam.G.copy(), fam.c.copy()
    if what == "nan_diagonal":
        G[5, 5] = np.nan
    else:
        G[9, :] = 0.0
        G[:, 9] = 0.0
        c[9] = 0.0
    ptr = buf.load(G, c)
    for kind, param in ((_capi.SOLVE_RIDGE, 0.0), (_capi.SOLVE_LSTSQ, RCOND), (_capi.SOLVE_CHOL, 0.0)):
        dev = outcome(lambda: ctx.solve_device(kind, param, K, ptr))
        host = outcome(lambda: _capi.solve(kind, param, G, c))
        print(f"chol gauss-K{K} {what} {KIND_NAMES[kind]}: device {dev[:2]} host {host[:2]}")
        assert dev[:2] == host[:2]
        if dev[0] == "ok":
            assert cc.same_bits(dev[2], host[2]) and (dev[3] == host[3] or (dev[3] != dev[3] and host[3] != host[3]))
            assert _capi.cond_info()[3] == 0


def test_status_word_survives_refused_factorisations():
    """The status word is cleared by the last launch of the previous chain and its address depends on K: good and refused
    factorisations of different widths in turn on ONE context."""
    c = _capi.HipContext(0)
    b = Buffer(c)
    c.set_option("device_solve", 1)
    try:
        def good(K):
            ref = cc.reference("gauss", K)
            device_solve(c, b.load(ref.G, ref.c), ref, _capi.SOLVE_LSTSQ, " (sequence)")

        def refused(K, kind):
            dup = cc.family("dup", K)
            beta, rank, _ = c.solve_device(kind, RCOND, K, b.load(dup.G, dup.c))
            return rank, _capi.cond_info()[3]

        good(257)
        assert refused(257, _capi.SOLVE_LSTSQ) == (256, 0)          # failed pivot -> general host path
        good(257)
        good(448)
        rank, _ = refused(448, _capi.SOLVE_LSTSQ_PROBE)
        assert rank == -1                                            # a probe comes straight back: unresolved
        good(257)
        good(129)
    finally:
        c.set_option("device_solve", 0)
        b.free()
        c.close()


# ---- 5. the factor-only form through lstsq_rows -----------------------------------------------------------------------------------

def lstsq_case(K, zero_column=None):
    m = 4 * K + 3
    A = cc.conditioned(m, K, 1.0e6, "geometric", K)
    r = np.random.default_rng(K)
    if zero_column is not None:
        A[:, zero_column] = 0.0
    b = A @ r.standard_normal(K) + 1.0e-3 * r.standard_normal(m)
    w = r.uniform(0.5, 2.0, m)
    return A, b, w


def both_routes(A, b, w, monkeypatch, capfd):
    """fsnap_lstsq_rows with the pass factor from the device (launch_chol_factor) and from the host (device_solve = 2)."""
    monkeypatch.setenv("FSNAP_ROWSPACE_TIMING", "1")
    c = _capi.HipContext(0)
    try:
        c.upload_rows(A, b)
        c.set_weights(w)
        capfd.readouterr()
        dev = c.lstsq_rows(RCOND)
        marks = capfd.readouterr().err
        assert "factor (device)" in marks and "factor_pass" not in marks, marks
        c.set_option("device_solve", 2)
        host = c.lstsq_rows(RCOND)
        marks = capfd.readouterr().err
        assert "factor_pass" in marks and "factor (device)" not in marks, marks
    finally:
        c.close()
    return dev, host


@pytest.mark.parametrize("K", cc.LSTSQ_K)
def test_factor_only_form_through_lstsq_rows(K, monkeypatch, capfd):
    """K padded to 16 equal to K padded to 64 (384, 640) and not (385, 400, 449, 513); kappa = 1e6, so two passes run."""
    A, b, w = lstsq_case(K)
    (beta, rank, info), (beta_h, rank_h, info_h) = both_routes(A, b, w, monkeypatch, capfd)
    want = orc.svd_fit(A, b, w)
    kw = np.linalg.cond(w[:, None] * A)
    bar = max(1.0e-6, 50.0 * kw * EPS)
    err = np.linalg.norm(beta - want) / np.linalg.norm(want)
    gap = np.linalg.norm(beta - beta_h) / np.linalg.norm(want)
    print(f"chol lstsq_rows K{K} K16 {cc.pad(K, 16)} np {cc.pad(K)}: passes {info['passes']:.0f} deviation {info['deviation']:.2e} "
          f"err/bar {err / bar:.3g} device-host/bar {gap / bar:.3g}")
    assert rank == rank_h == K
    assert info["passes"] == info_h["passes"] >= 2 and info["converged"] == info_h["converged"] == 1.0
    assert info["deviation"] <= 1.0e-10 and info_h["deviation"] <= 1.0e-10
    assert err <= bar and gap <= bar


def test_factor_only_form_with_an_inactive_column(monkeypatch, capfd):
    """An all-zero column inside the last 16-block (unit row and column in the factor) at K16 != np."""
    K, z = 400, 395
    A, b, w = lstsq_case(K, zero_column=z)
    (beta, rank, info), (beta_h, rank_h, info_h) = both_routes(A, b, w, monkeypatch, capfd)
    print(f"chol lstsq_rows K{K} zero column {z}: rank {rank} / {rank_h} passes {info['passes']:.0f} / {info_h['passes']:.0f}")
    assert rank == rank_h
    assert beta[z] == 0.0 and beta_h[z] == 0.0
    want = orc.svd_fit(A, b, w)
    keep = np.arange(K) != z
    bar = max(1.0e-6, 50.0 * np.linalg.cond(w[:, None] * A[:, keep]) * EPS)
    assert np.linalg.norm(beta - want) <= bar * np.linalg.norm(want)
    assert np.linalg.norm(beta - beta_h) <= bar * np.linalg.norm(want)
