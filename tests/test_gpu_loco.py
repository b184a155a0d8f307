"""GPU: exact leave-one-configuration-out predictions (fsnap_loco_rows, csrc/fsnap_loco.hip; Solver.loco_errors) against
long-double refits (tests/loco_cases.py) under an a-priori rounding bar and an RMS comparison with loco_host: a sweep of K,
J (J = K and J < K factors) and unit sizes on every tile and bin edge, interleaved / strided / caller-owned layouts, more
units than workgroups, the pivot decision across LOCO_PIVOT_TOL, class-level fits with J < K and on the row-space path; the
Ta golden rows (leave-one-group-out against lstsq), a column that one configuration alone touches, determinism, residency,
two ranks and 10^6 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import loco, solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loco_cases import (EPS, LAM_MIN, LD_ALL_BELOW, RMS_FACTOR, SWEEP_ALPHA, SWEEP_K, Refit, cell_line,  # noqa: E402
                        config_rows, downdated, measure_cell, stats_ld, sweep_factor, sweep_js, sweep_rows, sweep_units,
                        unit_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def kernel(A, b, w, mask, M, beta, labels):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w, None if mask is None else mask.astype(np.uint8))
    train = np.ones(len(b), dtype=bool) if mask is None else mask.astype(bool)
    rows, off, units = loco.unit_index(labels, train)
    pred, info = ctx.loco_rows(M, beta, rows, off)
    ctx.close()
    return pred, info, rows, off, units


def check_cell(tag, A, b, w_eff, alpha, M, beta, rows, off, pred, info, stats=None, ld_units=None, ld_bars=True):
    """Every assertion of one (K, alpha, J) cell on the kernel's output, after printing the cell's line of the measured
    table.  Returns measure_cell's dict."""
    J = M.shape[1]
    n = np.diff(off)
    host, hinfo = loco.loco_host(A, b, w_eff, M, beta, rows, off)
    res = measure_cell(A, b, w_eff, alpha, M, beta, rows, off, pred, stats, ld_units, host, ld_bars)
    print(cell_line(tag, res), flush=True)
    assert np.all(info[:, 2] == 1.0)
    assert np.array_equal(info[:, 0], np.minimum(n, J))
    assert np.array_equal(info[:, 3], (n <= J).astype(float))
    assert np.array_equal(res["d"], np.minimum(n, J)) and np.array_equal(res["nspace"], n <= J)
    assert np.min(res["lam_min"]) >= LAM_MIN, (tag, np.min(res["lam_min"]))
    have = np.isfinite(res["piv"])
    assert np.all(np.abs(info[have, 1] - res["piv"][have]) <= 4 * (J + res["d"][have]) * EPS), tag
    np.testing.assert_allclose(info[:, 1], hinfo[:, 1], rtol=1e-8, atol=1e-12)
    listed = rows[:off[-1]]
    assert np.max(res["abs"]) <= 1e-9 * np.max(np.abs(b)), tag
    assert np.max(np.abs(pred[listed] - host[listed])) <= 1e-9 * np.max(np.abs(b)), tag
    worst = int(np.argmax(res["ratio"]))
    assert res["ratio"][worst] <= 1.0, (tag, "unit", worst, "rows", int(n[worst]), res["ratio"][worst])
    assert res["rms_pred"] <= RMS_FACTOR * res["rms_host"], (tag, res["rms_pred"], res["rms_host"])
    return res


def upload(A, b, w, mask=None):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w, None if mask is None else mask.astype(np.uint8))
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("K", SWEEP_K)
@pytest.mark.parametrize("alpha", SWEEP_ALPHA)
def test_kernel_matches_brute_force_refits(K, alpha):
    """Every row of every unit of the sweep of loco_cases (unit sizes on every tile and bin edge and at J - 1, J, J + 1, in
    shuffled order; J = K and the J < K of sweep_js) against the long-double refit, under the a-priori bar and the RMS
    condition; at K >= 256 the refits cover the boundary-size units and loco_host the fillers."""
    A, b, w, G, c, stats = sweep_rows(K)
    m = len(b)
    rows = np.arange(m, dtype=np.int32)
    ctx = upload(A, b, w)
    try:
        for J in sweep_js(K):
            off, boundary = sweep_units(K, J, m)
            M, beta = sweep_factor(G, c, alpha, J, stats)
            pred, info = ctx.loco_rows(M, beta, rows, off)
            check_cell(f"sweep K={K} alpha={alpha:g} J={J}", A, b, w, alpha, M, beta, rows, off, pred, info, stats,
                       None if K < LD_ALL_BELOW else boundary)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_zero_weight_and_testing_rows():
    A, b, w, labels = config_rows(3, 31, [20, 40, 25, 60, 35, 30, 45])
    w[::7] = 0.0
    mask = np.ones(len(b), dtype=bool)
    mask[3::11] = False
    w_eff = np.where(mask, w, 0.0)
    Aw, bw = A * w_eff[:, None], b * w_eff
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-6 * np.eye(31), Aw.T @ bw)
    M = loco.factor_cholesky(G, 1e-6)
    pred, info, rows, off, _ = kernel(A, b, w, mask, M, beta, labels["Configs"])
    assert np.all(np.isnan(pred[~mask]))
    cfg = np.asarray(labels["Configs"])
    for u in dict.fromkeys(labels["Configs"]):
        r = np.flatnonzero((cfg == u) & mask)
        ref = downdated(A, b, w_eff, r, 1e-6)
        assert np.max(np.abs(pred[r] - ref)) <= 1e-9 * np.max(np.abs(b))


@pytest.mark.gpu
def test_leave_one_group_out_on_ta_rows_matches_lstsq_refits(ta, ta_fits):
    A, b, w = ta
    groups = ta_fits["ea_groups"]
    m = len(b)
    fs = {"Groups": groups.tolist(), "Testing": [False] * m, "Row_Type": ["Energy" if i % 5 == 0 else "Force" for i in range(m)],
          "Configs": [f"c{i // 7}" for i in range(m)]}
    pt, s = make_solver("SVD")
    s.perform_fit(A, b, w, fs_dict=fs)
    res = s.loco_errors(by="Groups", fs_dict=fs, b=b, w=w)
    assert res.unidentifiable == 0
    Aw, bw = A * w[:, None], b * w
    eps = np.finfo(float).eps
    for g in sorted(set(groups)):
        out = groups == g
        beta = np.linalg.lstsq(Aw[~out], bw[~out], rcond=1e-13)[0]
        ref = A[out] @ beta
        kappa = np.linalg.cond(Aw[~out])
        rel = np.max(np.abs(res.preds[out] - ref)) / np.max(np.abs(ref))
        assert rel <= max(1e-6, 50 * kappa * eps), (g, rel, kappa)
    # the *ALL training rows of the LOO table next to error_analysis's in-sample ones: same row layout
    s.error_analysis(A, b, w, fs_dict=fs)
    assert list(res.errors.index) == list(s.errors.index)
    pt.free()


@pytest.mark.gpu
def test_a_column_one_configuration_alone_touches():
    A, b, w, labels = config_rows(11, 31, [30, 25, 40, 35, 50, 45])
    cfg = np.asarray(labels["Configs"])
    A[:, 7] = 0.0
    A[cfg == "cfg2", 7] = 1.0 + 0.05 * np.arange(40)
    Aw, bw = A * w[:, None], b * w
    G = Aw.T @ Aw
    for alpha, ident in ((0.0, 0.0), (1e-4, 1.0)):
        beta = np.linalg.solve(G + alpha * np.eye(31), Aw.T @ bw)
        pred, info, rows, off, units = kernel(A, b, w, None, loco.factor_cholesky(G, alpha), beta, labels["Configs"])
        u = units.index("cfg2")
        assert info[u, 2] == ident
        assert np.all(np.delete(info[:, 2], u) == 1.0)
        if ident:
            assert np.all(np.isfinite(pred))
            r = rows[off[u]:off[u + 1]]
            assert np.max(np.abs(pred[r] - downdated(A, b, w, r, alpha))) <= 1e-8 * np.max(np.abs(b))
        else:
            assert np.all(np.isnan(pred[cfg == "cfg2"])) and np.all(np.isfinite(pred[cfg != "cfg2"]))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142, 290])
def test_interleaved_units_strided_rows_and_caller_owned_weights(K):
    """One combined layout case: units interleaved over the rows (unit of row i = i % 7) and assigned at random, rows in a
    strided view (lda = K + 5), weights and mask in caller-owned device memory (bind_weights), a 10 % testing mask and
    zero-weight training rows inside n-space and J-space units.  Both bars hold, and every row has the bits of the
    contiguous, unit-sorted upload of the same rows."""
    import torch

    rng = np.random.default_rng(300 + K)
    m = 700 + max(1400, 5 * K + 150)
    big = rng.standard_normal((m, K + 5))
    big[:, :K] *= rng.uniform(0.5, 2.0, K)
    A = big[:, :K]
    assert A.strides[0] == 8 * (K + 5)
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    w[::11] = 0.0
    unit = np.arange(m) % 7
    # at random: one large unit (J space at every K), 19 of medium size and 12 of a dozen rows
    unit[700:] = 7 + rng.choice(32, m - 700, p=[0.25] + [0.63 / 19] * 19 + [0.01] * 12)
    labels = [f"u{u}" for u in unit]
    mask = rng.random(m) >= 0.1
    w_eff = np.where(mask, w, 0.0)
    stats = stats_ld(A, b, w_eff)
    Aw = A * w_eff[:, None]
    G, c = Aw.T @ Aw, Aw.T @ (b * w_eff)
    rows, off, _ = loco.unit_index(labels, mask)
    n = np.diff(off)
    assert n.max() > K and n.min() <= min(K, 32) and (K <= 32 or np.any((n > 32) & (n <= K)))
    assert np.any(w_eff[rows[off[np.argmax(n)]:off[np.argmax(n) + 1]]] == 0.0)
    alpha = 1e-8
    factors = [sweep_factor(G, c, alpha, J, stats) for J in (K, (K // 2) | 1)]
    dev = torch.device("cuda", 0)
    dw = torch.from_numpy(w).to(dev)
    dm = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    torch.cuda.synchronize()
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.bind_weights(dw.data_ptr(), dm.data_ptr())
    preds = []
    try:
        for M, beta in factors:
            pred, info = ctx.loco_rows(M, beta, rows, off)
            assert np.all(np.isnan(pred[~mask])) and np.all(np.isfinite(pred[mask]))
            check_cell(f"layout K={K} J={M.shape[1]}", A, b, w_eff, alpha, M, beta, rows, off, pred, info, stats)
            preds.append((pred, info))
    finally:
        ctx.close()
    # the same rows contiguous and unit-sorted (the testing rows behind them), weights through set_weights
    order = np.concatenate([rows, np.flatnonzero(~mask)])
    ctx = upload(np.ascontiguousarray(A[order]), b[order], w[order], mask[order])
    try:
        for (M, beta), (pred, info) in zip(factors, preds):
            p2, i2 = ctx.loco_rows(M, beta, np.arange(len(rows), dtype=np.int32), off)
            assert np.array_equal(p2, pred[order], equal_nan=True) and np.array_equal(i2, info)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 48])
def test_workgroups_reuse_their_buffers_over_twenty_thousand_units(K):
    """More units than workgroups (16 per compute unit) in the LDS bins: a workgroup runs a smaller unit after a larger one
    in the same sH, sr and vbuf.  K = 31 keeps every unit in the 32 bin (d_c <= 31); K = 48 fills the 32 and the 64 bin.
    Every unit against loco_host under the a-priori bar, 64 of them against the long-double refit."""
    import torch

    rng = np.random.default_rng(40 + K)
    J = K
    ncfg = 20_000
    sizes = rng.choice(sorted(set(range(1, 41)) | {J, J + 1}), ncfg)
    m = int(sizes.sum())
    A = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    nwg = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    d = np.minimum(sizes, J)
    assert np.count_nonzero(d <= 32) > nwg and (K == 31 or np.count_nonzero(d > 32) > nwg)
    stats = stats_ld(A, b, w)
    Aw = A * w[:, None]
    G, c = Aw.T @ Aw, Aw.T @ (b * w)
    M, beta = sweep_factor(G, c, 0.0, J, stats)
    rows = np.arange(m, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ctx = upload(A, b, w)
    try:
        pred, info = ctx.loco_rows(M, beta, rows, off)
    finally:
        ctx.close()
    ld = np.zeros(ncfg, dtype=bool)
    ld[rng.choice(ncfg, 64, replace=False)] = True
    check_cell(f"reuse K={K} J={J}", A, b, w, 0.0, M, beta, rows, off, pred, info, stats, ld, ld_bars=False)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_the_pivot_decision_near_the_tolerance(K):
    """A column that one unit nearly alone touches (its entries in the other rows scaled by epsilon), for a unit in n space
    and one in J space: epsilon steps the smallest pivot of the reference H_c through 1e-6 ... 1e-12 and 0, across
    LOCO_PIVOT_TOL = 1e-10.  The reported pivot, the decision, the predictions of the identifiable units (under the a-priori
    bar, which its 1 / lambda_min term widens here) and the NaN rows of the refused ones."""
    sizes = [20, 50, 40, 45, 35, 60, 55] if K == 31 else [100, 200, 150, 150, 150, 150, 150]
    A0, b, w, _ = config_rows(50 + K, K, sizes)
    m = len(b)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    cols = (7, K - 3)                                   # the column of unit 0 (n space), of unit 1 (J space)
    rows = np.arange(m, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    J = K

    def system(eps):
        A = A0.copy()
        for u, col in enumerate(cols):
            A[cfg != u, col] *= eps[u]
        stats = stats_ld(A, b, w)
        Aw = A * w[:, None]
        M, beta = sweep_factor(Aw.T @ Aw, Aw.T @ (b * w), 0.0, J, stats)
        return A, stats, M, beta

    def unit_ref(A, M, beta, u):
        return unit_reference(A, b, w, rows[off[u]:off[u + 1]], M, beta)

    # the pivot is proportional to epsilon^2 for a small epsilon: one probe per unit sets the scale
    A, _, M, beta = system((1e-3, 1e-3))
    scale = [unit_ref(A, M, beta, u)["piv"] / 1e-6 for u in (0, 1)]
    seen = []
    for target in (1e-6, 1e-8, 1e-9, 1e-11, 1e-12, 0.0):
        A, stats, M, beta = system([np.sqrt(target / scale[u]) for u in (0, 1)])
        pred, info, *_ = kernel(A, b, w, None, M, beta, cfg.tolist())
        refit = Refit(A, b, w, 0.0, None, stats)
        assert np.array_equal(info[:, 0], np.minimum(sizes, J)) and np.array_equal(info[:2, 3], [1.0, 0.0])
        for u in range(len(sizes)):
            r = rows[off[u]:off[u + 1]]
            ref = unit_ref(A, M, beta, u)
            bound = 4 * (J + ref["d"]) * EPS
            print(f"LOCO pivot K={K} target {target:g} unit {u}: reference pivot {ref['piv']:.6g}, kernel {info[u, 1]:.6g}, "
                  f"identifiable {info[u, 2]:g}, lam_min {ref['lam_min']:.3g}", flush=True)
            assert abs(info[u, 1] - ref["piv"]) <= bound, (target, u, info[u, 1], ref["piv"])
            if abs(ref["piv"] - loco.PIVOT_TOL) > bound:
                assert info[u, 2] == float(ref["piv"] > loco.PIVOT_TOL), (target, u)
            if u < 2:
                seen.append(ref["piv"])
                if target > 0.0:
                    assert 0.5 * target <= ref["piv"] <= 2.0 * target, (target, u, ref["piv"])
                else:
                    assert abs(ref["piv"]) <= bound
                    assert info[u, 2] == 0.0
            else:
                assert info[u, 2] == 1.0
            if info[u, 2] == 1.0:
                err = np.abs(pred[r] - refit.predict(r))
                assert np.all(np.isfinite(pred[r]))
                print(f"LOCO pivot K={K} target {target:g} unit {u}: worst err/bar {np.max(err / ref['bar']):.3g}", flush=True)
                assert np.all(err <= ref["bar"]), (target, u, np.max(err / ref["bar"]))
            else:
                assert np.all(np.isnan(pred[r]))
    assert min(seen) < loco.PIVOT_TOL < max(seen)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 142])
def test_bit_identical_repeats_and_permutation_of_configurations(K):
    sizes = [10, 33, 130, 64, 200, 17, 150, 150]
    A, b, w, labels = config_rows(2, K, sizes)
    Aw = A * w[:, None]
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-6 * np.eye(K), Aw.T @ (b * w))
    M = loco.factor_cholesky(G, 1e-6)
    p1, i1, *_ = kernel(A, b, w, None, M, beta, labels["Configs"])
    p2, i2, *_ = kernel(A, b, w, None, M, beta, labels["Configs"])
    assert np.array_equal(p1, p2) and np.array_equal(i1, i2)
    # the configurations' row blocks in another order (rows within a configuration keep their order)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    order = np.concatenate([np.flatnonzero(cfg == c) for c in np.random.default_rng(0).permutation(len(sizes))])
    p3, *_ = kernel(A[order], b[order], w[order], None, M, beta, [labels["Configs"][i] for i in order])
    assert np.array_equal(p3, p1[order])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["RIDGE", "SVD", "ANL"])
def test_resident_rows_stay_and_a_following_fit_is_unchanged(name):
    A, b, w, labels = config_rows(9, 31, [15 + (5 * c) % 60 for c in range(30)], testing_frac=0.1)
    pt, s = make_solver(name, {"RIDGE": {"alpha": 1e-6}} if name == "RIDGE" else None)
    if name == "ANL":
        pt.create_shared_array("a", *A.shape)
        pt.create_shared_array("b", len(b))
        pt.create_shared_array("w", len(b))
        pt.shared_arrays["a"].array[:] = A
        pt.shared_arrays["b"].array[:] = b
        pt.shared_arrays["w"].array[:] = w
        pt.fitsnap_dict = dict(labels)
        s.save_files = False
        s.perform_fit()
        fit1 = np.array(s.fit)
        res = s.loco_errors()
        s.perform_fit()
    else:
        test = np.asarray(labels["Testing"])
        s.keep_resident = True
        s.perform_fit(A, b, w[~test], fs_dict=labels)
        fit1 = np.array(s.fit)
        res = s.loco_errors(fs_dict=labels, b=b, w=w[~test])
        s.perform_fit(A, b, w[~test], fs_dict=labels)
    assert np.array_equal(np.asarray(s.fit), fit1)
    assert res.unidentifiable == 0
    assert np.all(np.isnan(res.preds[np.asarray(labels["Testing"])]))
    assert np.all(np.isfinite(res.preds[~np.asarray(labels["Testing"])]))
    assert len(res.units) == 30 and np.all(res.units["identifiable"])
    pt.free()


def class_case(case):
    """(A, b, w, labels) of the class-level cases with fewer kept directions than columns, or a fit on the rows."""
    rng = np.random.default_rng(len(case))
    if case == "svd_row_space":                     # one singular value of 1e-8: tests/test_gpu_rowspace.py's family
        m, K, cycle = 6000, 64, [1, 5, 17, 63, 64, 65, 100, 130]
        U, _ = np.linalg.qr(rng.standard_normal((m, K)))
        V, _ = np.linalg.qr(rng.standard_normal((K, K)))
        sv = np.ones(K)
        sv[-1] = 1e-8
        A = (U * sv) @ V.T
        noise = 1e-3
    else:                                           # rank 30 of 34: three duplicated columns and an exactly zero one
        m, cycle = 3000, [1, 5, 17, 29, 30, 31, 64, 100]
        base = rng.standard_normal((m, 30)) * rng.uniform(0.5, 2.0, 30)
        A = np.hstack([base, base[:, :3], np.zeros((m, 1))])
        noise = 0.05
    b = A @ rng.standard_normal(A.shape[1]) + noise * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    sizes = []
    while sum(sizes) < m:
        sizes.append(min(cycle[len(sizes) % len(cycle)], m - sum(sizes)))
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    labels = {"Configs": [f"cfg{c}" for c in cfg], "Groups": [f"g{c % 3}" for c in cfg], "Testing": [False] * m,
              "Row_Type": [("Energy", "Force", "Stress")[i % 3] for i in range(m)]}
    return np.ascontiguousarray(A), b, w, labels


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["svd_row_space", "svd_rank_deficient", "anl_rank_deficient"])
def test_loco_errors_of_fits_with_a_factor_from_smoother_factor(case):
    """Solver.loco_errors after an SVD fit through the row-space path, after a rank-deficient SVD fit and after ANL on
    rank-deficient rows (J < K in the last two), against the long-double refit in the projected features of the M that
    smoother_factor returns; bar: the a-priori bar plus max(1e-6, 50 kappa eps) relative for the fit's own beta."""
    A, b, w, labels = class_case(case)
    m, K = A.shape
    name = "ANL" if case.startswith("anl") else "SVD"
    pt, s = make_solver(name)
    if name == "ANL":
        pt.create_shared_array("a", m, K)
        pt.create_shared_array("b", m)
        pt.create_shared_array("w", m)
        pt.shared_arrays["a"].array[:] = A
        pt.shared_arrays["b"].array[:] = b
        pt.shared_arrays["w"].array[:] = w
        pt.fitsnap_dict = dict(labels)
        s.save_files = False
        s.perform_fit()
        res = s.loco_errors()
    else:
        s.perform_fit(A, b, w, fs_dict=labels)
        res = s.loco_errors(fs_dict=labels, b=b, w=w)
    M = loco.smoother_factor(s, loco.rows_triangle(A, w))[1]
    beta = np.asarray(s.fit, dtype=np.float64).reshape(-1)
    J = M.shape[1]
    if case == "svd_row_space":
        assert s.last_row_space is not None and K - 1 <= J <= K
    else:
        assert J == 30
    assert res.unidentifiable == 0 and np.all(res.units["identifiable"])
    rows, off, units = loco.unit_index(labels["Configs"], np.ones(m, dtype=bool))
    n = np.diff(off)
    assert list(res.units["Configs"]) == units
    assert np.array_equal(res.units["d"].to_numpy(), np.minimum(n, J))
    sv = np.linalg.svd(A * w[:, None], compute_uv=False)
    kappa = sv[0] / sv[J - 1]
    rel = max(1e-6, 50 * kappa * EPS)
    refit = Refit(A, b, w, 0.0, M, projected=True, project_rows=True)
    worst = 0.0
    for u in range(len(units)):
        r = rows[off[u]:off[u + 1]]
        ref = unit_reference(A, b, w, r, M, beta)
        truth = refit.predict(r, ref["zeta"])
        assert ref["lam_min"] >= LAM_MIN
        ratio = np.max(np.abs(res.preds[r] - truth) / (ref["bar"] + rel * np.max(np.abs(truth))))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, u, len(r), ratio)
    print(f"LOCO class {case}: J = {J} of K = {K}, kappa {kappa:.3g}, worst error / bar {worst:.3g}", flush=True)
    pt.free()


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="loco two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "loco_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"loco_rank{r}.npz")) for r in range(world)]
    sizes = [12 + (7 * c) % 90 for c in range(40)]
    A, b, w, labels = config_rows(5, 31, sizes, testing_frac=0.1)
    test = np.asarray(labels["Testing"])
    # per row, bit for bit: the same M and beta on one context holding all rows
    M, beta = parts[0]["M"], parts[0]["beta"]
    assert np.array_equal(parts[1]["M"], M) and np.array_equal(parts[1]["beta"], beta)
    one, *_ = kernel(A, b, w, (~test), M, beta, labels["Configs"])
    for p in parts:
        assert np.array_equal(p["preds"], one[p["rows"]], equal_nan=True)
    # tables: one rank's own fit and LOCO
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": 1e-6}})
    s.perform_fit(A, b, w[~test], fs_dict=labels)
    res = s.loco_errors(fs_dict=labels, b=b, w=w[~test])
    assert [str(x) for x in res.errors.index] == parts[0]["index"].tolist()
    np.testing.assert_allclose(parts[0]["errors"], res.errors.to_numpy(dtype=float), rtol=1e-12, atol=0)
    pt.free()


@pytest.mark.gpu
def test_million_rows_ten_thousand_configurations():
    rng = np.random.default_rng(0)
    K = 128
    sizes = rng.integers(32, 171, 10_000)
    m = int(sizes.sum())
    A = rng.standard_normal((m, K))
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    Aw = A * w[:, None]
    G, c = Aw.T @ Aw, Aw.T @ (b * w)
    beta = np.linalg.solve(G, c)
    M = loco.factor_cholesky(G)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pred, info = ctx.loco_rows(M, beta, np.arange(m, dtype=np.int32), off)
    ctx.close()
    assert np.all(info[:, 2] == 1.0) and np.all(np.isfinite(pred))
    for u in rng.choice(len(sizes), 12, replace=False):
        r = np.arange(off[u], off[u + 1])
        ref = downdated(A, b, w, r, 0.0, G, c)
        assert np.max(np.abs(pred[r] - ref)) <= 1e-9 * np.max(np.abs(b)), u
    assert m >= 10**6
    # every unit against loco_host under the a-priori bar
    check_cell("million K=128", A, b, w, 0.0, M, beta, np.arange(m, dtype=np.int32), off, pred, info, None,
               np.zeros(len(sizes), dtype=bool), ld_bars=False)


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "loco_validation.py")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "*ALL" in r.stdout
