"""GPU: the leave-one-unit-out ridge alpha path (fsnap_ridge_path, csrc/fsnap_path.hip; Solver.ridge_path) against the
long-double refit of tests/loco_cases.py under the a-priori bar of tests/ridge_path_cases.py, the numpy form
(ridge_path_host), the Woodbury route (fsnap_loco_rows) and brute-force refits; layouts, determinism, refusals, two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, solver_factory
from fitsnap_amd.solvers import ridge_path as rp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loco_cases as lc  # noqa: E402
import ridge_path_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = lc.EPS


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def upload(A, b, w, mask=None):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w, None if mask is None else mask.astype(np.uint8))
    return ctx


def stats_of(A, b, w_eff):
    Aw = A * w_eff[:, None]
    return Aw.T @ Aw, Aw.T @ (b * w_eff)


def kernel(A, b, w, mask, alphas, labels, classes=None, nclass=1, G=None, c=None):
    """fsnap_ridge_path on a fresh context: (sums, info, preds, rows, off, units)."""
    m = len(b)
    train = np.ones(m, dtype=bool) if mask is None else mask.astype(bool)
    if G is None:
        G, c = stats_of(A, b, np.where(train, w, 0.0))
    rows, off, units = loco.unit_index(labels, train)
    ctx = upload(A, b, w, mask)
    try:
        sums, info, preds = ctx.ridge_path(G, c, alphas, rows, off, np.zeros(m, np.uint8) if classes is None else classes,
                                           nclass, want_preds=True)
    finally:
        ctx.close()
    return sums, info, preds, rows, off, units


def check_sums(b, w_eff, sums, preds, rows, off, cls, nclass):
    """The kernel's sums against the sums of its own predictions recomputed on the host: within n_u eps of the terms."""
    for q in range(sums.shape[0]):
        for u in range(len(off) - 1):
            r = rows[off[u]:off[u + 1]]
            own = rc.own_sums(b, w_eff, preds[q], r, cls, nclass)
            assert np.all(np.abs(sums[q, u] - own) <= len(r) * EPS * np.abs(own)), (q, u, sums[q, u], own)


@pytest.mark.gpu
@pytest.mark.parametrize("K", rc.SWEEP_K)
def test_kernel_matches_the_long_double_refit_over_the_geometry_sweep(K):
    """Rows of loco_cases.sweep_rows(K), units of sweep_units(K, K, m) (sizes on the MFMA k-steps of 4 and the 16-row tiles,
    K - 1, K, K + 1, fillers of 150), Q = 5 alphas {0, 1e-8, 1e-4, 1, 1e2}, 3 row classes.  No unit is flagged; per (K, alpha)
    the kernel's RMS error against the long-double refit is at most RMS_FACTOR x ridge_path_host's (boundary-size units; the
    fillers are compared with ridge_path_host); every row is within ridge_path_cases.kernel_bar; the sums are those of the
    kernel's own predictions to n_u eps.  Every cell prints its line (profiles/ridge_path_accuracy.txt)."""
    lc.need_long_double()
    A, b, w, G, c, stats = lc.sweep_rows(K)
    m = len(b)
    off, boundary = lc.sweep_units(K, K, m)
    rows = np.arange(m, dtype=np.int32)
    cls = rc.row_classes(m)
    ctx = upload(A, b, w)
    try:
        sums, info, preds = ctx.ridge_path(G, c, rc.ALPHAS, rows, off, cls, rc.NCLASS, want_preds=True)
    finally:
        ctx.close()
    hsums, hinfo, hpreds = rp.ridge_path_host(A, b, w, G, c, rc.ALPHAS, rows, off, cls, rc.NCLASS)
    res = rc.measure(A, b, w, stats, rows, off, rc.ALPHAS, preds, hpreds, boundary)
    for q, alpha in enumerate(rc.ALPHAS):
        print(rc.cell_line(K, alpha, res, q), flush=True)
    assert np.all(hinfo[:, :, 1] == 1.0) and np.all(info[:, :, 1] == 1.0)
    np.testing.assert_allclose(info[:, :, 0], hinfo[:, :, 0], rtol=1e-8, atol=1e-12)
    assert np.all(np.isfinite(preds))
    for q, alpha in enumerate(rc.ALPHAS):
        worst = int(np.argmax(res["ratio"][q]))
        assert res["ratio"][q, worst] <= 1.0, (K, alpha, "unit", worst, "rows", int(off[worst + 1] - off[worst]))
        assert res["rms_pred"][q] <= lc.RMS_FACTOR * res["rms_host"][q], (K, alpha, res["rms_pred"][q], res["rms_host"][q])
    check_sums(b, w, sums, preds, rows, off, cls, rc.NCLASS)
    assert np.array_equal(sums[:, :, :, 0], hsums[:, :, :, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 16, 17])
def test_grid_sizes_around_the_chunk_of_sixteen_and_duplicate_alphas(Q):
    A, b, w, labels = lc.config_rows(21, 33, [5, 40, 17, 70, 33, 34, 150])
    alphas = np.logspace(-8, 2, Q)
    if Q > 1:
        alphas[-1] = alphas[0]                      # a duplicate, in another chunk when Q = 17
        alphas[Q // 2] = 0.0
    cls = rc.row_classes(len(b))
    sums, info, preds, rows, off, _ = kernel(A, b, w, None, alphas, labels["Configs"], cls, rc.NCLASS)
    G, c = stats_of(A, b, w)
    hsums, hinfo, hpreds = rp.ridge_path_host(A, b, w, G, c, alphas, rows, off, cls, rc.NCLASS)
    assert np.all(info[:, :, 1] == 1.0)
    assert np.max(np.abs(preds - hpreds)) <= 1e-10 * np.max(np.abs(b))
    np.testing.assert_allclose(sums, hsums, rtol=1e-9, atol=1e-12)
    if Q > 1:
        assert np.array_equal(preds[-1], preds[0]) and np.array_equal(sums[-1], sums[0]) and np.array_equal(info[-1], info[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["RIDGE", "SVD"])
def test_solver_path_agrees_with_loco_errors_and_with_the_woodbury_route(name):
    """At the solver's own alpha the refit predictions agree with Solver.loco_errors(...).preds (the Woodbury form of the
    same quantity), and method="woodbury" agrees with method="refit" on every alpha, within the sum of the two a-priori bars
    (loco_cases.kernel_bar and ridge_path_cases.kernel_bar, from long-double intermediates)."""
    lc.need_long_double()
    K = 31
    A, b, w, labels = lc.config_rows(8, K, [9, 31, 40, 16, 64, 33, 120, 7, 50])
    own = 1e-6 if name == "RIDGE" else 0.0
    pt, s = make_solver(name, {"RIDGE": {"alpha": own}} if name == "RIDGE" else None)
    s.keep_resident = True
    s.perform_fit(A, b, w, fs_dict=labels)
    alphas = [own, 1e-3, 10.0]
    ref = s.ridge_path(alphas, fs_dict=labels, b=b, w=w, method="refit", want_preds=True)
    woo = s.ridge_path(alphas, fs_dict=labels, b=b, w=w, method="woodbury", want_preds=True)
    auto = s.ridge_path(alphas, fs_dict=labels, b=b, w=w, want_preds=True)
    lo = s.loco_errors(fs_dict=labels, b=b, w=w)
    pt.free()
    assert np.array_equal(auto.preds, ref.preds) and auto.table.equals(ref.table)
    assert ref.unidentifiable.tolist() == [0, 0, 0] and woo.unidentifiable.tolist() == [0, 0, 0]
    stats = lc.stats_ld(A, b, w)
    G, c = stats_of(A, b, w)
    rows, off, _ = loco.unit_index(labels["Configs"], np.ones(len(b), dtype=bool))
    Ms = [loco.factor_cholesky(G, alpha) for alpha in alphas]          # the factors and fits the Woodbury passes were given
    worst = [0.0, 0.0]
    for u in range(len(off) - 1):
        r = rows[off[u]:off[u + 1]]
        refs = rc.unit_ld(A, b, w, stats, r, alphas)
        for q, alpha in enumerate(alphas):
            beta = np.asarray(s.fit).reshape(-1) if q == 0 else Ms[q] @ (Ms[q].T @ c)
            bar = rc.kernel_bar(A[r], refs[q]) + lc.unit_reference(A, b, w, r, Ms[q], beta)["bar"]
            worst[0] = max(worst[0], float(np.max(np.abs(woo.preds[q, r] - ref.preds[q, r]) / bar)))
            if q == 0:
                worst[1] = max(worst[1], float(np.max(np.abs(lo.preds[r] - ref.preds[0, r]) / bar)))
    print(f"PATH {name}: woodbury - refit over the sum of the bars {worst[0]:.3g}; loco_errors - refit {worst[1]:.3g}", flush=True)
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    np.testing.assert_allclose(woo.table.to_numpy(dtype=float), ref.table.to_numpy(dtype=float), rtol=1e-9)
    # the fits on all rows
    for q, alpha in enumerate(alphas):
        np.testing.assert_allclose(ref.fits[q], np.linalg.solve(G + alpha * np.eye(K), c), rtol=1e-8)


@pytest.mark.gpu
def test_zero_weight_rows_a_unit_of_weight_zero_and_testing_rows():
    A, b, w, labels = lc.config_rows(3, 31, [20, 40, 25, 60, 35, 30, 45])
    cfg = np.asarray(labels["Configs"])
    w[::7] = 0.0
    w[cfg == "cfg2"] = 0.0                          # a unit whose rows all have weight 0: predicted by the full fit
    mask = np.ones(len(b), dtype=bool)
    mask[3::11] = False
    w_eff = np.where(mask, w, 0.0)
    alphas = [1e-6, 1e-2]
    sums, info, preds, rows, off, units = kernel(A, b, w, mask, alphas, labels["Configs"])
    assert np.all(np.isnan(preds[:, ~mask])) and np.all(np.isfinite(preds[:, mask])) and np.all(info[:, :, 1] == 1.0)
    G, c = stats_of(A, b, w_eff)
    for q, alpha in enumerate(alphas):
        for u in dict.fromkeys(labels["Configs"]):
            r = np.flatnonzero((cfg == u) & mask)
            assert np.max(np.abs(preds[q, r] - lc.downdated(A, b, w_eff, r, alpha))) <= 1e-9 * np.max(np.abs(b))
        r = np.flatnonzero((cfg == "cfg2") & mask)
        full = A[r] @ np.linalg.solve(G + alpha * np.eye(31), c)
        assert np.max(np.abs(preds[q, r] - full)) <= 1e-10 * np.max(np.abs(b))
        u = units.index("cfg2")
        assert sums[q, u, 0, 0] == len(r) and sums[q, u, 0, 3] == 0.0 and sums[q, u, 0, 2] > 0.0


@pytest.mark.gpu
def test_a_column_one_unit_alone_touches():
    lc.need_long_double()
    A, b, w, labels = lc.config_rows(11, 31, [30, 25, 40, 35, 50, 45])
    cfg = np.asarray(labels["Configs"])
    A[:, 7] = 0.0
    A[cfg == "cfg2", 7] = 1.0 + 0.05 * np.arange(40)
    sums, info, preds, rows, off, units = kernel(A, b, w, None, [0.0, 1e-4], labels["Configs"])
    u = units.index("cfg2")
    assert info[0, u, 1] == 0.0 and np.all(np.delete(info[0, :, 1], u) == 1.0) and np.all(info[1, :, 1] == 1.0)
    assert np.all(np.isnan(preds[0, cfg == "cfg2"])) and np.all(np.isfinite(preds[0, cfg != "cfg2"]))
    assert np.all(sums[0, u] == 0.0) and np.all(np.isfinite(preds[1]))
    r = rows[off[u]:off[u + 1]]
    ref = rc.unit_ld(A, b, w, lc.stats_ld(A, b, w), r, [1e-4])[0]
    assert ref["beta"][7] == 0.0                    # nothing but alpha is left on that column: its coefficient is 0
    assert np.max(np.abs(preds[1, r] - ref["pred"])) <= 1e-8 * np.max(np.abs(b))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_interleaved_units_strided_rows_and_caller_owned_weights(K):
    """Units interleaved over the rows, rows in a strided view (lda = K + 5), weights and mask in caller-owned device memory,
    a 10 % testing mask and zero-weight rows: every row has the bits of the contiguous, unit-sorted upload of the same rows,
    and agrees with ridge_path_host."""
    import torch

    rng = np.random.default_rng(300 + K)
    m = 2100
    big = rng.standard_normal((m, K + 5))
    big[:, :K] *= rng.uniform(0.5, 2.0, K)
    A = big[:, :K]
    assert A.strides[0] == 8 * (K + 5)
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    w[::11] = 0.0
    unit = np.arange(m) % 7
    unit[700:] = 7 + rng.choice(32, m - 700, p=[0.25] + [0.63 / 19] * 19 + [0.01] * 12)
    labels = [f"u{u}" for u in unit]
    mask = rng.random(m) >= 0.1
    w_eff = np.where(mask, w, 0.0)
    G, c = stats_of(A, b, w_eff)
    rows, off, _ = loco.unit_index(labels, mask)
    cls = rc.row_classes(m)
    dev = torch.device("cuda", 0)
    dw = torch.from_numpy(w).to(dev)
    dm = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    torch.cuda.synchronize()
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.bind_weights(dw.data_ptr(), dm.data_ptr())
    try:
        sums, info, preds = ctx.ridge_path(G, c, rc.ALPHAS, rows, off, cls, rc.NCLASS, want_preds=True)
    finally:
        ctx.close()
    assert np.all(np.isnan(preds[:, ~mask])) and np.all(np.isfinite(preds[:, mask])) and np.all(info[:, :, 1] == 1.0)
    hsums, _, hpreds = rp.ridge_path_host(A, b, w_eff, G, c, rc.ALPHAS, rows, off, cls, rc.NCLASS)
    assert np.max(np.abs(preds[:, mask] - hpreds[:, mask])) <= 1e-9 * np.max(np.abs(b))
    check_sums(b, w_eff, sums, preds, rows, off, cls, rc.NCLASS)
    order = np.concatenate([rows, np.flatnonzero(~mask)])
    ctx = upload(np.ascontiguousarray(A[order]), b[order], w[order], mask[order])
    try:
        s2, i2, p2 = ctx.ridge_path(G, c, rc.ALPHAS, np.arange(len(rows), dtype=np.int32), off, cls[order], rc.NCLASS,
                                    want_preds=True)
    finally:
        ctx.close()
    assert np.array_equal(p2, preds[:, order], equal_nan=True) and np.array_equal(i2, info) and np.array_equal(s2, sums)


@pytest.mark.gpu
def test_workgroups_reuse_their_buffers_over_twenty_thousand_units():
    """More units than workgroups: a workgroup runs unit after unit in the same LDS and scratch slice (K = 17, 20 000 units
    of 1 - 3 rows).  No unit is flagged; 200 sampled units per alpha against the float64 downdated solve; the row counts of
    every unit; the pooled sums of all units against the kernel's own predictions."""
    rng = np.random.default_rng(57)
    K, nu = 17, 20_000
    sizes = rng.integers(1, 4, nu)
    m = int(sizes.sum())
    A = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    G, c = stats_of(A, b, w)
    rows = np.arange(m, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    alphas = [0.0, 1e-4, 1.0]
    ctx = upload(A, b, w)
    try:
        sums, info, preds = ctx.ridge_path(G, c, alphas, rows, off, np.zeros(m, np.uint8), 1, want_preds=True)
    finally:
        ctx.close()
    assert np.all(info[:, :, 1] == 1.0)
    for q, alpha in enumerate(alphas):
        for u in rng.choice(nu, 200, replace=False):
            r = rows[off[u]:off[u + 1]]
            assert np.max(np.abs(preds[q, r] - lc.downdated(A, b, w, r, alpha, G, c))) <= 1e-10 * np.max(np.abs(b))
    r_all = b[None, :] - preds
    np.testing.assert_allclose(sums[:, :, 0, 2].sum(axis=1), (r_all ** 2).sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(sums[:, :, 0, 3].sum(axis=1), ((w[None, :] * r_all) ** 2).sum(axis=1), rtol=1e-12)
    assert np.array_equal(sums[:, :, 0, 0], np.broadcast_to(sizes, (3, nu)))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_bit_identical_repeats_and_permutation_of_units(K):
    sizes = [10, 33, 130, 64, 200, 17, 150, 150]
    A, b, w, labels = lc.config_rows(2, K, sizes)
    G, c = stats_of(A, b, w)
    cls = rc.row_classes(len(b))
    alphas = [1e-6, 0.0, 1.0]
    s1, i1, p1, *_ = kernel(A, b, w, None, alphas, labels["Configs"], cls, rc.NCLASS, G, c)
    s2, i2, p2, *_ = kernel(A, b, w, None, alphas, labels["Configs"], cls, rc.NCLASS, G, c)
    assert np.array_equal(p1, p2) and np.array_equal(i1, i2) and np.array_equal(s1, s2)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    perm = np.random.default_rng(0).permutation(len(sizes))
    order = np.concatenate([np.flatnonzero(cfg == u) for u in perm])
    s3, i3, p3, *_ = kernel(A[order], b[order], w[order], None, alphas, [labels["Configs"][i] for i in order], cls[order],
                            rc.NCLASS, G, c)
    assert np.array_equal(p3, p1[:, order]) and np.array_equal(s3, s1[:, perm]) and np.array_equal(i3, i1[:, perm])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["RIDGE", "SVD"])
def test_resident_rows_stay_and_a_following_fit_is_unchanged(name):
    A, b, w, labels = lc.config_rows(9, 31, [15 + (5 * u) % 60 for u in range(30)], testing_frac=0.1)
    pt, s = make_solver(name, {"RIDGE": {"alpha": 1e-6}} if name == "RIDGE" else None)
    test = np.asarray(labels["Testing"])
    s.keep_resident = True
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    fit1 = np.array(s.fit)
    res = s.ridge_path([1e-8, 1e-4, 1.0], fs_dict=labels, b=b, w=w[~test], want_preds=True)
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    assert np.array_equal(np.asarray(s.fit), fit1)
    assert res.unidentifiable.tolist() == [0, 0, 0]
    assert np.all(np.isnan(res.preds[:, test])) and np.all(np.isfinite(res.preds[:, ~test]))
    assert len(res.units) == 90 and np.all(res.units["identifiable"])
    assert res.best is not None and res.best_alpha == res.alphas[res.best]
    pt.free()


@pytest.mark.gpu
def test_wider_systems_take_the_composed_route_and_the_entry_point_refuses_them():
    K = 145
    A, b, w, labels = lc.config_rows(4, K, [30, 200, 150, 160, 180, 40])
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": 1e-6}})
    s.keep_resident = True
    s.perform_fit(A, b, w, fs_dict=labels)
    res = s.ridge_path([1e-6, 1e-2], fs_dict=labels, b=b, w=w, want_preds=True)
    with pytest.raises(ValueError, match="K <= 144"):
        s.ridge_path([1e-6], fs_dict=labels, b=b, w=w, method="refit")
    ctx = pt.hip()
    G, c = stats_of(A, b, w)
    rows, off, _ = loco.unit_index(labels["Configs"], np.ones(len(b), dtype=bool))
    with pytest.raises((ValueError, _capi.FsnapError)):
        ctx.ridge_path(G, c, [1e-6], rows, off, np.zeros(len(b), np.uint8), 1)
    cfg = np.asarray(labels["Configs"])
    for q, alpha in enumerate([1e-6, 1e-2]):
        for u in dict.fromkeys(labels["Configs"]):
            r = np.flatnonzero(cfg == u)
            assert np.max(np.abs(res.preds[q, r] - lc.downdated(A, b, w, r, alpha))) <= 1e-8 * np.max(np.abs(b))
    pt.free()


@pytest.mark.gpu
def test_entry_point_argument_checks():
    A, b, w, labels = lc.config_rows(6, 5, [4, 6, 5])
    G, c = stats_of(A, b, w)
    rows, off, _ = loco.unit_index(labels["Configs"], np.ones(len(b), dtype=bool))
    cls = rc.row_classes(len(b))
    ctx = upload(A, b, w)
    try:
        for bad in ([-1.0], [np.nan], [1.0, np.inf], []):
            with pytest.raises((ValueError, _capi.FsnapError)):
                ctx.ridge_path(G, c, bad, rows, off, cls, rc.NCLASS)
        for nclass in (0, 9, 2):                     # 2: the rows hold class 2
            with pytest.raises((ValueError, _capi.FsnapError)):
                ctx.ridge_path(G, c, [1.0], rows, off, cls, nclass)
        with pytest.raises((ValueError, _capi.FsnapError)):
            ctx.ridge_path(np.eye(4), np.ones(4), [1.0], rows, off, cls, rc.NCLASS)
        sums, info, preds = ctx.ridge_path(G, c, [1.0], rows, off, cls, rc.NCLASS)
        assert preds is None and np.all(info[:, :, 1] == 1.0)
        # a unit without rows between the others: zero sums, info (inf, 1), the others unchanged
        off2 = np.array([off[0], off[1], off[1], off[2], off[3]], dtype=np.int64)
        s2, i2, _ = ctx.ridge_path(G, c, [1.0, 0.0], rows, off2, cls, rc.NCLASS)
        assert np.all(s2[:, 1] == 0.0) and np.all(i2[:, 1, 0] == np.inf) and np.all(i2[:, 1, 1] == 1.0)
        assert np.array_equal(s2[0, [0, 2, 3]], sums[0]) and np.array_equal(i2[0, [0, 2, 3]], info[0])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_interior_minimum_through_the_solver():
    A, b, w, labels, alphas = rc.interior_case()
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": 1e-4}})
    s.keep_resident = True
    s.perform_fit(A, b, w, fs_dict=labels)
    res = s.ridge_path(alphas, fs_dict=labels, b=b, w=w)
    pt.free()
    assert res.best_alpha == 10.0 and res.best == 7 and not res.unidentifiable.any()
    hsums, hinfo, *_, names, _ = rc.host_path(A, b, w, alphas, labels)
    pooled, _ = rp.pool_sums(hsums, hinfo)
    host = rp.path_table(alphas, pooled, names)
    assert list(res.table.index) == list(host.index)
    allrows = [k for k in host.index if k[1] == "*ALL"]
    np.testing.assert_allclose(res.table.loc[allrows, "w_rmse"].to_numpy(), host.loc[allrows, "w_rmse"].to_numpy(), rtol=1e-11)
    curve = 60 * res.table.loc[allrows, "w_rmse"].to_numpy() ** 2
    assert np.all(np.abs(curve[[0, 7, 8]] - [1049.47, 972.29, 1777.9]) <= [0.005, 0.005, 0.05]), curve
    np.testing.assert_allclose(res.units["w_sse"].to_numpy().reshape(10, 12).sum(axis=1), curve, rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["RIDGE", "SVD"])
def test_leave_one_group_out_on_ta_rows_matches_refits(ta, ta_fits, name):
    """Through the solver objects on the golden Ta rows by="Groups", alpha in {0, 1e-8, 1e-4}: the predictions match
    np.linalg.lstsq (alpha = 0) / ridge refits without each group, to the tolerance of test_gpu_loco.py's Ta test."""
    A, b, w = ta
    groups = ta_fits["ea_groups"]
    m = len(b)
    fs = {"Groups": groups.tolist(), "Testing": [False] * m, "Row_Type": ["Energy" if i % 5 == 0 else "Force" for i in range(m)],
          "Configs": [f"c{i // 7}" for i in range(m)]}
    pt, s = make_solver(name, {"RIDGE": {"alpha": 1e-8}} if name == "RIDGE" else None)
    s.keep_resident = True
    s.perform_fit(A, b, w, fs_dict=fs)
    alphas = [0.0, 1e-8, 1e-4]
    res = s.ridge_path(alphas, by="Groups", fs_dict=fs, b=b, w=w, want_preds=True)
    pt.free()
    assert res.unidentifiable.tolist() == [0, 0, 0]
    Aw, bw = A * w[:, None], b * w
    eps = np.finfo(float).eps
    for g in sorted(set(groups)):
        out = groups == g
        kappa = np.linalg.cond(Aw[~out])
        for q, alpha in enumerate(alphas):
            if alpha == 0.0:
                beta = np.linalg.lstsq(Aw[~out], bw[~out], rcond=1e-13)[0]
            else:
                d = np.sqrt(np.sum(Aw[~out] ** 2, axis=0) + alpha)
                S = (Aw[~out].T @ Aw[~out] + alpha * np.eye(A.shape[1])) / d[:, None] / d[None, :]
                beta = np.linalg.solve(S, (Aw[~out].T @ bw[~out]) / d) / d
            ref = A[out] @ beta
            rel = np.max(np.abs(res.preds[q, out] - ref)) / np.max(np.abs(ref))
            assert rel <= max(1e-6, 50 * kappa * eps), (g, alpha, rel, kappa)
    assert set(res.table.index.get_level_values(1)) == {"*ALL", "Energy", "Force"}
    assert res.table.loc[(0.0, "*ALL")]["ncount"] == m


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="ridge path two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ridge_path_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"path_rank{r}.npz")) for r in range(world)]
    sizes = [12 + (7 * u) % 90 for u in range(40)]
    A, b, w, labels = lc.config_rows(5, 31, sizes, testing_frac=0.1)
    test = np.asarray(labels["Testing"])
    alphas = parts[0]["alphas"]
    G, c = parts[0]["G"], parts[0]["c"]
    assert np.array_equal(parts[1]["G"], G) and np.array_equal(parts[1]["c"], c)
    # one context that holds all rows, with the statistics the ranks used: the same bits per row, per unit and in the table
    names = sorted(set(labels["Row_Type"]))
    cls = np.array([names.index(t) for t in labels["Row_Type"]], dtype=np.uint8)
    sums, info, preds, rows, off, units = kernel(A, b, np.where(test, 0.0, w), ~test, alphas, labels["Configs"], cls,
                                                 len(names), G, c)
    for p in parts:
        assert np.array_equal(p["preds"], preds[:, p["rows"]], equal_nan=True)
    pooled, bad = rp.pool_sums(sums, info, units)
    one = rp.path_table(alphas, pooled, names)
    assert [str(x) for x in one.index] == parts[0]["index"].tolist()
    for p in parts:                                  # every rank holds the table
        assert np.array_equal(p["table"], one.to_numpy(dtype=float), equal_nan=True)
        assert p["best"] == rp.pick_best(alphas, pooled[:, :, 3].sum(axis=1), bad)
    assert sorted(parts[0]["unit_names"].tolist()) == sorted(f"{a:g}|{u}" for a in alphas for u in units)


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ridge_alpha_path.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "best alpha" in r.stdout and "*ALL" in r.stdout
