"""CPU: the a-priori bars of tests/trsm_cases.py are neither loose nor wrong, on the shapes tests/test_gpu_trsm.py uses.

For every shape of the GPU sweeps (family, first, kind, m, K): the fault-free float64 mirror of the family's kernel stays at
or below 1.0 bars, backward and forward; Q* R gives back X to long-double rounding; on benign and illblock factors the
forward bar of every entry is at most 1e-9 of the largest |q*| of its row; the factors that kernel 13B meets keep the
condition of every 16 x 16 diagonal block under 1e7; every fault of the mirror that can act on the shape lands more than 100
bars outside on at least one of the two bars.  No shape and no factor kind is left out.
A failing condition means fixing the inputs of trsm_cases.py, never loosening a bar."""
import numpy as np
import pytest

import trsm_cases as tc

LD = tc.LD


def grouped():
    """The sweep's cases by (family, K): one factor set per test."""
    groups = {}
    for fam, first, kind, m, K in tc.sweep_cases():
        groups.setdefault((fam, K), []).append((first, kind, m))
    return groups


GROUPS = grouped()


def test_sweeps_run_every_template_instance_and_every_panel_geometry():
    cases = tc.sweep_cases()
    names = {tc.instance(fam, first, K) for fam, first, kind, m, K in cases}
    want = {f"fsnap_trsm_acc2_k<{nb}, {f}>" for nb in range(1, 10) for f in ("true", "false")}
    want |= {f"fsnap_trsm_panel_k<{tr}, {kg}, {f}>" for tr, kg in ((1, 64), (2, 16)) for f in ("true", "false")}
    assert names == want
    assert all(tc.family_runs(fam, K) for fam, first, kind, m, K in cases)
    # kernel 13C: a last block of 1 and of 16 columns at every NB, of 14 or 15 at most of them
    widths = {(tc.k16_of(K) // 16, K - tc.k16_of(K) + 16) for K in tc.C_COLS}
    assert widths >= {(nb, w) for nb in range(1, 10) for w in (1, 16)} and len({nb for nb, w in widths if w in (14, 15)}) >= 6
    # kernel 13B: a last panel of 1 ... 8 blocks with 2, 3 and 4 panels each; 13 panels; K = K16 and K16 - 15 everywhere
    geo = {((tc.k16_of(K) // 16 + 7) // 8, (tc.k16_of(K) // 16 - 1) % 8 + 1) for K in tc.B_COLS}
    assert geo >= {(2, n) for n in range(1, 9)} and {n for p, n in geo if p == 3} == set(range(1, 9))
    assert (4, 1) in geo and (13, 4) in geo
    for k16 in range(144, 401, 16):
        assert k16 in tc.B_COLS and k16 - 15 in tc.B_COLS
    assert tc.C_COLS_M == 3 * 64 + 37 and tc.B_COLS_M == {2: 165, 3: 293}
    # the dispatch cases sit on both sides of the rule's two switches
    assert {(m, K): fam for m, K, fam in tc.DISPATCH} == {(m, K): tc.rule(m, K) for m, K, fam in tc.DISPATCH}
    assert {fam for m, K, fam in tc.DISPATCH} == {1, 2, 3}


def test_every_fault_acts_somewhere_in_every_family_it_belongs_to():
    seen = {}
    for fam, first, kind, m, K in tc.sweep_cases():
        case = tc.make_case(m, K, kind, first)
        for f in tc.FAULTS:
            if tc.fault_acts(f, fam, case):
                seen.setdefault(fam, set()).add(f)
    assert seen[tc.FAMILY_13C] == set(tc.FAULTS) - {"col_ge_k_next_row"}
    assert seen[tc.FAMILY_13B16] == seen[tc.FAMILY_13B32] == set(tc.FAULTS) - {"reciprocal_f32"}


def test_inverse_block_port_and_reference_pieces():
    fac = tc.factor(45, "illblock")
    Rpad = np.eye(48)
    Rpad[:45, :45] = fac.R
    inv = tc.invert_diagonal_blocks(Rpad)
    for jb in range(3):
        T = Rpad[16 * jb:16 * jb + 16, 16 * jb:16 * jb + 16]
        assert np.max(np.abs(inv[jb] @ T - np.eye(16))) < 1e-10 and not np.tril(inv[jb], -1).any()
    assert np.max(np.abs(tc._inverse_ld(fac.R) @ fac.R.astype(LD) - np.eye(45))) < 1e-15
    assert 5e3 < fac.cond_t < 2e4
    # first-pass inputs: NaN / Inf exactly in the rows of zero effective weight, the forced rows alive
    case = tc.make_case(229, 31, "benign", True)
    assert not np.isfinite(case.A[case.dead]).any() and np.isfinite(case.A[~case.dead]).all()
    assert case.dead.sum() > 40 and not case.dead[case.forced].any() and case.forced == [0, 63, 192, 228]
    assert np.isnan(case.A[case.dead]).any() and np.isposinf(case.A[case.dead]).any() and np.isneginf(case.A[case.dead]).any()
    assert (case.w[case.mask] == 0).any() and (~case.mask).sum() > 20
    ref = tc.reference(case)
    assert not ref.q[case.dead].any() and not np.signbit(ref.q[case.dead].astype(np.float64)).any()
    later = tc.make_case(229, 31, "benign", False)
    assert not later.X[later.dead].any() and np.isfinite(later.X).all()


@pytest.mark.parametrize("fam,K", sorted(GROUPS, key=lambda g: (g[1], g[0])), ids=lambda v: str(v))
def test_mirror_within_the_bars_and_every_fault_far_outside(fam, K):
    for n, (first, kind, m) in enumerate(GROUPS[(fam, K)]):
        case = tc.make_case(m, K, kind, first)
        ref = tc.reference(case)
        clean = tc.score(case, tc.mirror(case, fam))
        print(f"{case.name} family {fam}: mirror bw {clean['bw']:.3f} fw {clean['fw']:.3f} cond(T) {case.fac.cond_t:.2g}")
        assert clean["bw"] <= 1.0 and clean["fw"] <= 1.0, clean
        if fam != tc.FAMILY_13C:
            assert case.fac.cond_t < 1.0e7
        # the reference reproduces X: its own residual is 2^-11 of the bar (asserted with a factor two)
        res = np.abs(ref.q @ case.R.astype(LD) - ref.x)
        assert np.all(res <= ref.bw_bar * 2.0 ** -10)
        # the bars are not vacuous
        live = ~case.dead[ref.rows]
        assert np.all(ref.bw_bar[live] > 0) and np.all(ref.fw_bar[live] > 0) and not ref.bw_bar[~live].any()
        if kind != "cholqr":
            assert np.all(ref.fw_bar <= 1e-9 * np.max(np.abs(ref.q), axis=1, keepdims=True).astype(np.float64))
        assert np.all(ref.bw_bar <= 1e-12 * ref.terms)
        for f in tc.FAULTS:
            if not tc.fault_acts(f, fam, case):
                continue
            hit = tc.score(case, tc.mirror(case, fam, f), forward_only_above=100.0)
            print(f"    {f}: bw {hit['bw']:.3g} fw {hit['fw']:.3g}")
            assert max(hit["bw"], hit["fw"]) > 100.0, (case.name, fam, f, hit)
