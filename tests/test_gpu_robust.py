"""GPU: the robust (IRLS) step kernels of csrc/fsnap_robust.hip against long double and the fp64 host rule, the session's
clean-up, ``Solver.robust_fit`` / the ``ROBUST`` plugin end to end, and two ranks on one GPU.  Cases, reference and bars:
tests/robust_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import robust, solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = rc.EPS
LD = rc.LD


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(y, dtype=np.float64).view(np.uint64))


def upload(A, b, w, mask=None):
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w, None if mask is None else mask.astype(np.uint8))
    return ctx


def make_solver():
    pt = ParallelTools()
    return pt, solver_factory.solver("ROBUST", pt, Config(pt, {"SOLVER": {"solver": "ROBUST"}}))


# ---- 1. the residual pass -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 17, 31, 32, 33, 64, 128, 129, 142, 288, 289, 300])
def test_residual_pass_matches_long_double(K):
    """e_i = w_i (b_i - a_i . beta) of kernel R1 for m in {1, 7, 8, 9, 253, 2049} (one row, the 8-row step edges, a ragged tail,
    more than one grid stride) under the a-priori bar 4 eps (K + 2) w_i (|a_i| . |beta| + |b_i|); 10 % test rows and zero
    weights with NaN in their rows give exactly 0."""
    ctx = _capi.HipContext(0)
    try:
        _check_residuals(ctx, K)
    finally:
        ctx.close()


def _check_residuals(ctx, K):
    for m in (1, 7, 8, 9, 253, 2049):
        rng = np.random.default_rng(100 * K + m)
        A = rng.standard_normal((m, K)) * 10.0 ** rng.uniform(-1, 1, K)
        beta = rng.standard_normal(K)
        b = A @ beta + rng.standard_normal(m)
        w = 10.0 ** rng.uniform(-2, 2, m)
        mask = rng.random(m) >= 0.1
        w[rng.random(m) < 0.1] = 0.0
        if m == 1:
            mask[:], w[:] = True, 2.5
        part = mask & (w > 0)
        Ad, bd = A.copy(), b.copy()
        Ad[~part] = np.nan                       # NaN in rows that do not take part reaches nothing
        bd[~mask] = np.nan
        ctx.upload_rows(Ad, bd)
        ctx.set_weights(w, mask.astype(np.uint8))
        ctx.robust_begin(None, 1)
        ctx.robust_residuals(beta)
        e = ctx.robust_download()["e"]
        ctx.robust_end()
        ref = rc.residual_reference(A, b, w, part, beta)
        bar = rc.residual_bar(A, b, w, beta)
        assert np.all(e[~part] == 0.0), (K, m)
        err = np.abs(e.astype(LD) - ref)
        assert np.all(err[part] <= bar[part]), (K, m, float(np.max(err[part] / bar[part])))


# ---- 2. the selection ------------------------------------------------------------------------------------------------------

def _values(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n)
    if kind == "duplicates":
        return rng.choice([-3.0, 1.5, 1.5, 2.0, -2.0, 0.0], size=n)
    if kind == "zeros":
        v = np.zeros(n)
        v[: n // 3] = rng.standard_normal(n // 3)           # more than half exactly zero
        return rng.permutation(v)
    if kind == "denormal":
        return rng.integers(-40, 40, size=n) * 5e-324
    if kind == "huge":
        return rng.choice([1e300, -1e300, 3e299, 1.0], size=n)
    if kind == "equal":
        return np.full(n, -0.75)
    if kind == "mixed":
        return np.concatenate([rng.standard_normal(n - n // 2), rng.integers(0, 3, size=n // 2) * 1e-310])[rng.permutation(n)]
    raise ValueError(kind)


def _selection_case(sizes, kinds, seed):
    rng = np.random.default_rng(seed)
    cat = np.concatenate([np.full(n, g, dtype=np.int32) for g, n in enumerate(sizes)])
    val = np.concatenate([_values(kinds[g % len(kinds)], n, rng) for g, n in enumerate(sizes)])
    order = rng.permutation(len(cat))
    return cat[order], val[order]


@pytest.mark.gpu
@pytest.mark.parametrize("ncat", [1, 3, 32])
def test_selection_is_exact(ncat):
    """s_g of kernel R2 equals 1.4826 * np.median(|e_dev[class]|) bit for bit: class sizes 0, 1, 2, 3, 255, 256, 257, 4097,
    heavy duplicates, exact zeros, denormals, 1e300, all values equal; test rows and zero weights hold 1e308."""
    base = [0, 1, 2, 3, 255, 256, 257, 4097]
    kinds = ["normal", "duplicates", "zeros", "denormal", "huge", "equal", "mixed"]
    if ncat == 1:
        variants = [([n], [k]) for n in base[1:] for k in kinds]
    elif ncat == 3:
        variants = [([4097, 0, 256], kinds[0:]), ([3, 257, 2], kinds[1:]), ([255, 1, 4097], kinds[2:]), ([256, 256, 257], kinds[3:])]
    else:
        variants = [([base[(g * 3 + 1) % 8] for g in range(32)], kinds), ([base[(g * 5) % 8] for g in range(32)], kinds[::-1])]
    ctx = _capi.HipContext(0)
    try:
        _check_selection(ctx, ncat, variants)
    finally:
        ctx.close()


def _check_selection(ctx, ncat, variants):
    for vi, (sizes, ks) in enumerate(variants):
        cat, val = _selection_case(sizes, ks, 17 * ncat + vi)
        rng = np.random.default_rng(vi)
        extra = 37                                            # rows that must not take part
        cat = np.concatenate([cat, rng.integers(0, ncat, extra).astype(np.int32)])
        val = np.concatenate([val, np.full(extra, 1e308)])
        m = len(val)
        mask = np.ones(m, dtype=bool)
        w = np.ones(m)
        mask[m - extra:m - extra // 2] = False
        w[m - extra // 2:] = 0.0
        part = mask & (w > 0)
        ctx.upload_rows(np.zeros((m, 1)), val)                # a . beta = 0: e = w b = b exactly
        ctx.set_weights(w, mask.astype(np.uint8))
        ctx.robust_begin(cat, ncat)
        ctx.robust_residuals(np.zeros(1))
        s, n = ctx.robust_scale()
        s2, n2 = ctx.robust_scale()
        e = ctx.robust_download()["e"]
        ctx.robust_end()
        assert same_bits(e[part], val[part]) and np.all(e[~part] == 0.0)
        want = np.array([1.4826 * np.median(np.abs(e[part & (cat == g)])) if np.any(part & (cat == g)) else 0.0 for g in range(ncat)])
        assert n.tolist() == [int(np.count_nonzero(part & (cat == g))) for g in range(ncat)], (ncat, vi)
        assert same_bits(s, want), (ncat, vi, s, want)
        assert same_bits(s, s2) and n.tolist() == n2.tolist()


@pytest.mark.gpu
def test_argument_and_state_errors():
    cs = rc.case(3000, 17)
    ctx = upload(cs.A, cs.b, cs.w, cs.mask)
    try:
        with pytest.raises(_capi.FsnapError):                 # no session
            ctx.robust_residuals(np.zeros(17))
        with pytest.raises(ValueError):
            ctx.robust_begin(np.zeros(cs.m, dtype=np.int32), _capi.ROBUST_MAX_CLASSES + 1)
        with pytest.raises(ValueError):
            ctx.robust_begin(np.zeros(cs.m, dtype=np.int32), 0)
        with pytest.raises(ValueError):
            ctx.robust_begin(cs.cat, 2)                        # a class id out of range
        ctx.robust_begin(cs.cat, 3)
        with pytest.raises(ValueError):
            ctx.robust_residuals(np.zeros(16))                # not the rows' width
        with pytest.raises(_capi.FsnapError):
            ctx.robust_scale()                                # no residuals yet
        ctx.robust_residuals(np.zeros(17))
        with pytest.raises(_capi.FsnapError):
            ctx.robust_reweight("huber", 1.345)               # no scales yet
        ctx.robust_scale()
        with pytest.raises(ValueError):
            ctx.robust_reweight(7, 1.0)                       # unknown loss
        with pytest.raises(ValueError):
            ctx.robust_reweight("huber", 0.0)
        with pytest.raises(ValueError):
            ctx.robust_reweight("huber", -1.0)
        ctx.robust_end()
        with pytest.raises(_capi.FsnapError):
            ctx.robust_scale()
    finally:
        ctx.close()
    empty = _capi.HipContext(0)
    try:
        with pytest.raises(_capi.FsnapError):                 # no rows
            empty.robust_begin(None, 1)
    finally:
        empty.close()


# ---- 3. the weights --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("loss", rc.LOSSES)
def test_weights_match_the_host_rule(loss):
    """From the device's own e and s: branch membership is the fp64 host rule's exactly (huber r == 1 inside, bisquare r == 0
    outside), |w r - w r_ref| <= 16 eps w against long double, exact counts, sums within 4 eps n of long double, two runs
    bit-identical; a class with scale 0 gets r = 1."""
    cs = rc.case(5000, 33)
    c = rc.DEFAULT_TUNE[loss]
    beta = rc.probe_beta(cs)
    ctx = upload(cs.A, cs.b, cs.w, cs.mask)
    try:
        ctx.robust_begin(cs.cat, 3)
        ctx.robust_residuals(beta)
        s, n = ctx.robust_scale()
        sums = ctx.robust_reweight(loss, c)
        d = ctx.robust_download(e=True, r=True, wr=True)
        sums2 = ctx.robust_reweight(loss, c)
        d2 = ctx.robust_download(e=True, r=True, wr=True)
        zs = np.array([s[0], 0.0, s[2]])
        sums0 = ctx.robust_reweight(loss, c, scale=zs)
        d0 = ctx.robust_download(e=False, r=True, wr=True)
        ctx.robust_end()
    finally:
        ctx.close()
    part, cat, w = cs.part, cs.cat, cs.w
    e, r, wr = d["e"], d["r"], d["wr"]
    assert same_bits(sums, sums2) and all(same_bits(d[k], d2[k]) for k in d)
    # rows that take no part: r = 1, the weight untouched
    assert np.all(r[~part] == 1.0) and same_bits(wr[~part], w[~part])
    rh, rhoh = robust.robust_weight(loss, c, s[cat], e)
    cs_ = c * s[cat]
    if loss == "huber":
        inside = np.abs(e) <= cs_
        assert np.all(r[part & inside] == 1.0) and np.all(r[part & ~inside] < 1.0 + EPS)
    if loss == "bisquare":
        inside = np.abs(e) < cs_
        assert np.all(r[part & ~inside] == 0.0) and np.all(r[part & inside] > 0.0)
    assert np.array_equal(r[part] < 1.0, rh[part] < 1.0) and np.array_equal(r[part] == 0.0, rh[part] == 0.0)
    rl, rhol = rc.ref_weight_vec(loss, c, s[cat], e)
    assert np.all(np.abs(wr.astype(LD) - w * rl)[part] <= 16 * EPS * w[part])
    for g in range(3):
        sel = part & (cat == g)
        ng = int(np.count_nonzero(sel))
        assert sums[g, 0] == ng == n[g]
        assert sums[g, 1] == np.count_nonzero(rh[sel] < 1.0) and sums[g, 2] == np.count_nonzero(rh[sel] == 0.0)
        for col, ref in ((3, np.sum(rl[sel] * rl[sel])), (4, np.sum(e[sel].astype(LD) ** 2)), (5, np.sum(rhol[sel]))):
            assert abs(LD(sums[g, col]) - ref) <= 4 * EPS * ng * ref, (loss, g, col)
    # scale 0: r = 1 and rho = 0 for the class, the others unchanged
    assert np.all(d0["r"][cat == 1] == 1.0) and same_bits(d0["wr"][cat == 1], w[cat == 1])
    assert sums0[1, 1] == 0 and sums0[1, 3] == sums0[1, 0] and sums0[1, 5] == 0.0
    assert same_bits(sums0[[0, 2]], sums[[0, 2]]) and same_bits(d0["wr"][cat != 1], wr[cat != 1])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [17, 128, 300])
def test_fused_launch_equals_separate_launches(K):
    cs = rc.case(2049, K) if K != 17 else rc.case(3000, 17)
    beta = rc.probe_beta(cs)
    fixed = np.array([0.1, 0.05, 0.02])
    ctx = upload(cs.A, cs.b, cs.w, cs.mask)
    try:
        ctx.robust_begin(cs.cat, 3)
        for loss in rc.LOSSES:
            c = rc.DEFAULT_TUNE[loss]
            ctx.robust_residuals(beta)
            sums = ctx.robust_reweight(loss, c, scale=fixed)
            sep = ctx.robust_download(e=True, r=True, wr=True)
            ctx.robust_residuals(np.zeros(K))                # (the fused launch must not live on the vectors above)
            fsums = ctx.robust_step(beta, loss, c, scale=fixed)
            fus = ctx.robust_download(e=True, r=True, wr=True)
            assert same_bits(sums, fsums), loss
            assert all(same_bits(sep[k], fus[k]) for k in sep), loss
        ctx.robust_end()
    finally:
        ctx.close()


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("loss", rc.LOSSES)
@pytest.mark.parametrize("m,K", rc.SHAPES)
def test_robust_fit_matches_long_double(m, K, loss):
    cs = rc.case(m, K)
    ref = rc.reference_of(m, K, loss)
    pt, s = make_solver()
    labels = cs.fs_dict()
    res = s.robust_fit(loss=loss, alpha=rc.ALPHA, max_iter=rc.FIXED_ITERS, tol=0.0, a=cs.A, b=cs.b, w=cs.w[cs.mask], fs_dict=labels)
    d = rc.distance(res.fit, ref["fit"])
    print(f"robust_fit vs long double, {m} x {K}, {loss}: {d:.3e} (bar {rc.gpu_bar(m, K, loss):.1e})")
    assert res.iterations == rc.FIXED_ITERS and res.classes == ["Energy", "Force", "Stress"]
    assert d <= rc.gpu_bar(m, K, loss)
    assert same_bits(s.fit, res.fit)
    assert np.array_equal(res.tables[:, :, 0], ref["tables"][:, :, 0].astype(float))
    assert np.max(np.abs(res.scales - ref["scales"].astype(float)) / ref["scales"].astype(float)) < 1e-9
    assert np.max(np.abs(res.omega() - ref["omega"].astype(float))) < 1e-7
    # tol = 1e-8: converged, as many iterations as the yardstick (within one)
    host = robust.robust_host(cs.A, cs.b, cs.w, cs.mask, cs.cat, loss=loss, alpha=rc.ALPHA, ncat=3)
    res2 = s.robust_fit(loss=loss, alpha=rc.ALPHA, a=cs.A, b=cs.b, w=cs.w[cs.mask], fs_dict=labels)
    assert res2.converged and host.converged and abs(res2.iterations - host.iterations) <= 1
    assert rc.distance(res2.fit, host.fit) < 1e-6
    pt.free()


@pytest.mark.gpu
def test_plugin_fixed_scale_scale_iters_and_table():
    cs = rc.case(3000, 17)
    labels = cs.fs_dict()
    args = dict(a=cs.A, b=cs.b, w=cs.w[cs.mask], fs_dict=labels)
    pt, s = make_solver()
    # the plugin class: [ROBUST] defaults = huber, per-row-type scales, tol 1e-8
    s.perform_fit(**args)
    host = robust.robust_host(cs.A, cs.b, cs.w, cs.mask, cs.cat, loss="huber", alpha=1e-8, ncat=3)
    assert s.robust.converged and abs(s.robust.iterations - host.iterations) <= 1
    assert rc.distance(s.fit, host.fit) < 1e-6
    planted = cs.outliers[cs.part[cs.outliers]]
    assert np.all(s.robust.omega()[planted] < 0.5)
    tab = s.robust.table(by="Configs")
    assert list(tab.columns) == ["Configs", "count", "mean_omega", "rejected", "downweighted"]
    assert tab["count"].sum() == int(cs.part.sum()) and tab["mean_omega"].is_monotonic_increasing
    worst = set(tab["Configs"][:20])
    assert worst <= {f"cfg{i // 13}" for i in planted}                  # the most suspect configurations hold planted outliers
    assert len(s.robust.table(by="Groups")) == 4
    # a fixed scale and scale_iters = 3 (their later iterations take the fused launch) against long double
    fixed = np.array([0.1, 0.05, 0.02])
    for kw in (dict(scale=fixed), dict(scale_iters=3)):
        ref = rc.reference(cs.A, cs.b, cs.w, cs.mask, cs.cat, 3, "bisquare", max_iter=6, **kw)
        res = s.robust_fit(loss="bisquare", alpha=rc.ALPHA, max_iter=6, tol=0.0, **kw, **args)
        assert rc.distance(res.fit, ref["fit"]) <= rc.gpu_bar(3000, 17, "bisquare"), kw
        assert np.array_equal(res.tables[:, :, :3], ref["tables"][:, :, :3].astype(float)), kw
        if "scale_iters" in kw:
            assert same_bits(res.scales[3], res.scales[2]) and same_bits(res.scales[5], res.scales[2])
        else:
            assert np.all(res.scales == fixed[None, :])
    # an explicit start and integer classes
    res = s.robust_fit(loss="cauchy", by=cs.cat, start=np.zeros(17), max_iter=30, **args)
    assert res.converged and np.all(res.start == 0.0) and res.classes == [0, 1, 2]
    with pytest.raises(ValueError):
        s.robust_fit(by=np.arange(cs.m) % 33, **args)                  # more classes than the kernels hold
    pt.free()


@pytest.mark.gpu
def test_python_m_fitsnap3_with_solver_robust_writes_a_potential(tmp_path, ta, monkeypatch):
    """`python -m fitsnap3` with `solver = ROBUST` on the golden Ta rows (no planted outliers): a potential and a metrics file
    come out, the coefficients are those of ``robust_host`` with the section's settings."""
    import runpy

    import pandas as pd

    from fitsnap_amd.io.outputs.snap import parse_snapcoeff
    from test_cli_cpu import TA_IN

    A, b, w = ta
    np.save(tmp_path / "Descriptors.npy", A)
    np.save(tmp_path / "Truth-Ref.npy", b)
    np.save(tmp_path / "Weights.npy", w)
    m = len(b)
    rtype = ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178
    pd.DataFrame({"Row_Type": rtype, "Groups": ["Ta"] * m, "Configs": ["c"] * m, "Testing": [False] * m, "Atom_I": [0] * m,
                  "Atom_Type": [0] * m}).to_pickle(tmp_path / "FitSNAP.df")
    text = TA_IN.replace("dump_descriptors = 1", "dump_descriptors = 0").replace("solver = SVD", "solver = ROBUST")
    (tmp_path / "Ta.in").write_text(text + "\n[ROBUST]\nloss = bisquare\nmax_iter = 30\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["fitsnap3", "Ta.in", "--descriptors", str(tmp_path), "--overwrite"])
    with pytest.raises(SystemExit) as e:
        runpy.run_module("fitsnap3", run_name="__main__", alter_sys=True)
    assert e.value.code == 0
    coeffs = parse_snapcoeff(tmp_path / "Ta_pot.snapcoeff")
    assert "('*ALL', 'Unweighted', 'Training', 'Energy')" in (tmp_path / "Ta_metrics.md").read_text()
    # the same rows through the plugin class in this process: the same launches, so the file holds that fit (18 digits).
    # (robust_host is no yardstick HERE: the Ta statistics span 30 decades, two fp64 normal-equation solvers differ by 1e-7
    # per fit on them and thirty re-weightings of a redescending loss carry that to 3e-4 of the coefficients.)
    pt = ParallelTools()
    s = solver_factory.solver("ROBUST", pt, Config(pt, {"SOLVER": {"solver": "ROBUST"}, "ROBUST": {"loss": "bisquare", "max_iter": 30}}))
    s.perform_fit(A, b, w, fs_dict={"Testing": [False] * m, "Row_Type": rtype})
    assert s.robust.loss == "bisquare" and s.robust.classes == ["Energy", "Force", "Stress"] and s.robust.iterations >= 2
    assert len(coeffs) == 31 and np.max(np.abs(coeffs - s.fit)) <= 1e-12 * np.max(np.abs(s.fit))
    pt.free()


# ---- 5. clean-up -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_session_leaves_the_context_as_it_was():
    cs = rc.case(3000, 17)
    labels = cs.fs_dict()
    pt, s = make_solver()
    args = dict(a=cs.A, b=cs.b, w=cs.w[cs.mask], fs_dict=labels)
    s.robust_fit(max_iter=1, **args)
    ctx = pt.hip()
    before = ctx.normal_eq()
    s.keep_resident = True
    s.robust_fit(loss="bisquare", max_iter=5, **args)
    after = ctx.normal_eq()
    assert all(same_bits(x, y) for x, y in zip(before, after))
    # a call that raises inside the session (the device refuses a beta of the wrong width) still ends it
    ctx.robust_begin(cs.cat, 3)
    try:
        ctx.robust_step(rc.probe_beta(cs), "huber", 1.345, scale=np.array([0.1, 0.05, 0.02]))
        changed = ctx.normal_eq()
        with pytest.raises(ValueError):
            ctx.robust_step(np.zeros(5), "huber", 1.345)
    finally:
        ctx.robust_end()
    assert not same_bits(changed[0], before[0])                        # inside the session the fits read w r
    assert all(same_bits(x, y) for x, y in zip(before, ctx.normal_eq()))
    with pytest.raises(ValueError):
        s.robust_fit(loss="huber", start=np.zeros(5), **args)
    with pytest.raises(ValueError):
        s.robust_fit(loss="l1", **args)
    assert all(same_bits(x, y) for x, y in zip(before, ctx.normal_eq()))
    pt.free()


# ---- 6. two ranks on one GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, monkeypatch):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="robust two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "robust_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    parts = [dict(np.load(tmp_path / f"robust_rank{r}.npz")) for r in range(world)]
    cs = rc.case(3000, 17)
    beta = rc.probe_beta(cs)
    ctx = upload(cs.A, cs.b, cs.w, cs.mask)
    try:
        ctx.robust_begin(cs.cat, 3)
        ctx.robust_residuals(beta)
        scale, count = ctx.robust_scale()
        ctx.robust_end()
    finally:
        ctx.close()
    monkeypatch.chdir(tmp_path)
    pt, s = make_solver()
    one = s.robust_fit(loss="huber", alpha=rc.ALPHA, max_iter=rc.FIXED_ITERS, tol=0.0, a=cs.A, b=cs.b, w=cs.w[cs.mask],
                       fs_dict=cs.fs_dict())
    ref = rc.reference_of(3000, 17, "huber")
    for deal in ("split", "empty"):
        for p in parts:
            assert same_bits(p[deal + "_scale"], scale) and p[deal + "_count"].tolist() == count.tolist(), deal
            assert rc.distance(p[deal + "_fit"], ref["fit"]) <= rc.gpu_bar(3000, 17, "huber"), deal
            assert rc.distance(p[deal + "_fit"], one.fit) <= rc.gpu_bar(3000, 17, "huber"), deal
            assert np.array_equal(p[deal + "_tables"][:, :, :3], one.tables[:, :, :3]), deal
            np.testing.assert_allclose(p[deal + "_omega"], one.omega()[p[deal + "_rows"]], rtol=0, atol=1e-8)
        assert same_bits(parts[0][deal + "_fit"], parts[1][deal + "_fit"])
        assert same_bits(parts[0][deal + "_scales"], parts[1][deal + "_scales"])
    assert len(parts[1]["empty_rows"]) == 0
    pt.free()
