"""CPU: the host side of the batched candidate fits (fitsnap_amd/solvers/candidates.py, fsnap_cat_chunks): the mapping of
GA-style group weights to per-category scales, the error sums assembled from per-category constants, the chunk layout of
the candidate kernels and the argument checks.  No GPU compute is called here."""
import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers.candidates import assemble_sums, category_constants, check_scales
from oracle import fitsnap_oracle as orc

ROW_TYPE = ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178


def make(name="SVD", sections=None):
    pt = ParallelTools()
    cfg = Config(pt, sections or {"SOLVER": {"solver": name}})
    return pt, solver_factory.solver(name, pt, cfg)


def ta_fs(ta_fits):
    return {"Groups": [str(g) for g in ta_fits["ea_groups"]], "Testing": ta_fits["testing_mask"].tolist(), "Row_Type": ROW_TYPE}


def update_weights_rows(table, groups, row_type):
    """The row loop of the reference's update_weights (libmod_optimize.py:407-417), restated."""
    new_w = np.zeros(len(groups))
    for i, (g, rt) in enumerate(zip(groups, row_type)):
        if rt == "Energy":
            new_w[i] = table[g]["eweight"]
        elif rt == "Force":
            new_w[i] = table[g]["fweight"]
        elif rt == "Stress":
            new_w[i] = table[g]["vweight"]
    return new_w


def test_scales_follow_update_weights_on_the_ta_labels(ta, ta_fits):
    A, b, _ = ta
    fs = ta_fs(ta_fits)
    _, s = make()
    cf = CandidateFits(s, A, b, fs_dict=fs)
    groups = sorted(set(fs["Groups"]))
    assert [k[0] for k in cf.keys] == sorted(k[0] for k in cf.keys) and len(cf.keys) == len(set(cf.keys))
    rng = np.random.default_rng(5)
    cands = []
    for _ in range(6):
        ew = 10.0 ** rng.uniform(-4, 4, len(groups))
        fr = 10.0 ** rng.uniform(-3, 3, len(groups))
        sr = 10.0 ** rng.uniform(-3, 3, len(groups))
        cands.append({g: {"eweight": ew[i], "fweight": ew[i] * fr[i], "vweight": ew[i] * sr[i]} for i, g in enumerate(groups)})
    S = cf.scales_from_group_weights(cands)
    assert S.shape == (6, cf.ncat)
    for p, table in enumerate(cands):
        ref = update_weights_rows(table, fs["Groups"], ROW_TYPE)
        assert np.array_equal(cf.row_weights(S[p]), ref)


def test_other_row_types_get_zero_scale():
    _, s = make()
    A = np.ones((4, 2))
    fs = {"Groups": ["a", "a", "b", "b"], "Testing": [False] * 4, "Row_Type": ["Energy", "Charge", "Force", "Stress"]}
    cf = CandidateFits(s, A, np.zeros(4), fs_dict=fs)
    S = cf.scales_from_group_weights([{"a": {"eweight": 2.0, "fweight": 3.0, "vweight": 4.0},
                                       "b": {"eweight": 5.0, "fweight": 6.0, "vweight": 7.0}}])
    assert np.array_equal(cf.row_weights(S[0]), [2.0, 0.0, 6.0, 7.0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_assembled_sums_match_the_oracle_error_rows(seed):
    rng = np.random.default_rng(seed)
    ncat = 7
    m = 400
    cat = rng.integers(0, ncat, m).astype(np.int32)
    cat[:5] = -1                                       # rows without a category take no part
    t = rng.standard_normal(m) * 10.0 ** rng.uniform(-2, 2)
    pred = t + rng.standard_normal(m) * 0.1
    w0 = 10.0 ** rng.uniform(-2, 2, m)
    w0[cat == 2] = 0.0                                 # a category whose base weights are all zero
    w0[rng.random(m) < 0.1] = 0.0
    s = 10.0 ** rng.uniform(-3, 3, ncat) * rng.choice([-1.0, 1.0], ncat)
    s[4] = 0.0                                         # a category the candidate switches off
    const = category_constants(t, w0, cat, ncat)
    r = t - pred
    sums4 = np.zeros((ncat, 4))
    for c in range(ncat):
        rc, wc = r[cat == c], w0[cat == c]
        sums4[c] = [np.abs(rc).sum(), (rc * rc).sum(), np.abs(wc * rc).sum(), ((wc * rc) ** 2).sum()]
    st = assemble_sums(const, sums4, s)
    got = Solver_metrics(st)
    for c in range(ncat):
        sel = cat == c
        ref = orc.error_row(t[sel], pred[sel], w0[sel] * s[c])
        for j, key in enumerate(("ncount", "mae", "rmse", "rsq", "w_ncount", "w_mae", "w_rmse", "w_rsq")):
            a, e = got[c, j], ref[key]
            if np.isnan(e):
                assert np.isnan(a), (c, key)
            elif key in ("rsq", "w_rsq"):
                assert abs(a - e) < 1e-11, (c, key, a, e)
            else:
                assert abs(a - e) <= 1e-12 * abs(e), (c, key, a, e)


def Solver_metrics(st):
    from fitsnap_amd.solvers.solver import Solver

    mm = Solver._metrics_from_sums(*(st[:, k] for k in range(10)))
    return np.column_stack([np.asarray(mm[c], dtype=np.float64) for c in Solver._METRIC_COLUMNS])


@pytest.mark.parametrize("masked", [False, True])
def test_chunk_layout_covers_every_row_once(masked):
    rng = np.random.default_rng(11)
    ncat = 9
    R = _capi.cat_limits()["chunk_rows"]
    sizes = {0: 0, 1: 1, 2: R, 3: R + 1, 4: 3 * R - 72, 5: 2, 6: 0, 7: 777, 8: 2 * R + 1}
    cat = np.concatenate([np.full(n, c, dtype=np.int32) for c, n in sizes.items()] + [np.full(13, -1, dtype=np.int32)])
    rng.shuffle(cat)
    mask = (rng.random(len(cat)) < 0.7).astype(np.uint8) if masked else None
    idx, ch = _capi.cat_chunks(cat, ncat, mask)
    take = (cat >= 0) & (mask.astype(bool) if masked else True)
    assert np.array_equal(np.sort(idx), np.flatnonzero(take))        # every row exactly once
    assert np.all(np.diff(ch[:, 0]) >= 0)                           # category order
    assert np.all((ch[:, 2] >= 1) & (ch[:, 2] <= R))                # no empty chunk, at most R rows
    assert np.array_equal(np.bincount(ch[:, 0], minlength=ncat),                  # the fewest chunks that hold them
                          [-(-int(np.count_nonzero(take & (cat == c))) // R) for c in range(ncat)])
    assert np.array_equal(ch[:, 1], np.concatenate([[0], np.cumsum(ch[:-1, 2])]))
    for c0, first, n in ch:
        rows = idx[first:first + n]
        assert np.all(cat[rows] == c0)                               # no chunk crosses a category
    for c in range(ncat):
        rows = np.concatenate([idx[f:f + n] for c0, f, n in ch if c0 == c] or [np.zeros(0, dtype=np.int32)])
        assert np.array_equal(rows, np.flatnonzero(take & (cat == c)))   # stable: ascending row ids
    empty = [c for c in range(ncat) if not np.any(take & (cat == c))]
    assert not set(empty) & set(ch[:, 0].tolist())


def test_chunk_layout_rejects_out_of_range_categories():
    with pytest.raises(ValueError):
        _capi.cat_chunks(np.array([0, 3, 1], dtype=np.int32), 3)


def test_argument_checks(ta, ta_fits):
    A, b, _ = ta
    fs = ta_fs(ta_fits)
    _, s = make()
    cf = CandidateFits(s, A, b, fs_dict=fs)
    with pytest.raises(ValueError, match="P = 0"):
        cf.fit(np.zeros((0, cf.ncat)))
    with pytest.raises(ValueError, match="shape"):
        cf.fit(np.ones((3, cf.ncat + 1)))
    with pytest.raises(ValueError, match="shape"):
        cf.errors(np.zeros((2, 31)), np.ones(cf.ncat))
    with pytest.raises(ValueError):
        check_scales(np.full((1, 2), np.nan), 2)
    with pytest.raises(ValueError, match="w0"):
        CandidateFits(s, A, b, w0=np.ones(5), fs_dict=fs)


@pytest.mark.parametrize("name", ["ARD", "LASSO", "ANL", "MERR"])
def test_unsupported_solvers_raise(name, ta, ta_fits):
    A, b, _ = ta
    _, s = make(name)
    with pytest.raises(NotImplementedError, match="SVD and RIDGE"):
        CandidateFits(s, A, b, fs_dict=ta_fs(ta_fits))


@pytest.mark.parametrize("name", ["SVD", "RIDGE"])
def test_apply_transpose_raises(name, ta, ta_fits):
    A, b, _ = ta
    _, s = make(name, {"SOLVER": {"solver": name}, "EXTRAS": {"apply_transpose": 1}})
    with pytest.raises(NotImplementedError, match="apply_transpose"):
        CandidateFits(s, A, b, fs_dict=ta_fs(ta_fits))


def test_kernel_sizes_come_from_the_library():
    # the row kernel's candidates per launch and the chunk length are the library's own (fsnap_cat_info without a context)
    lim = _capi.cat_limits()
    assert lim["chunk_rows"] == 1024 and lim["max_p"] == 16
