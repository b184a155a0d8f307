"""CPU: the a-priori bars of tests/rows_cases.py are neither loose nor wrong, on the shapes tests/test_gpu_rows.py uses.

For every shape: the fault-free float64 mirror stays at or below 1.0 bars in every output, every applicable fault of the
mirror lands more than 100 bars outside in at least one output, and every bar is at most 1e-9 of the sum of the absolute
terms of its quantity.  A failing condition means fixing the inputs of rows_cases.py, never loosening a bar.

Every shape is the GPU file's own (no subset: the long-double references of all of them take a few seconds together)."""
import numpy as np
import pytest

import rows_cases as rc

K_CASES = [(rc.sweep_m(K), K, None, True) for K in rc.K_SWEEP]
M_CASES = [(m, K, None, True) for K in rc.M_SWEEP_K for m in rc.M_SWEEP]
GRID = [(m, K, None, True) for m, K in rc.GRID_CASES]
LAYOUT = [(rc.LAYOUT_M, K, lda, True) for K, lda in rc.LAYOUT_CASES] + [(rc.LAYOUT_M, 31, None, False),
                                                                       (rc.LAYOUT_M, 300, None, False)]
GARBAGE = [(rc.GARBAGE_M, K, None, True) for K in rc.GARBAGE_K]
ALL = K_CASES + M_CASES + GRID + LAYOUT + GARBAGE
STATS = list(rc.STATS_CASES)


def ident(args):
    return "-".join(str(a) for a in args)


def test_shapes_reach_both_sides_of_every_launcher_switch():
    ks = set(rc.K_SWEEP)
    for edge in (8, 16, 32, 64, 128, 192, 224, 256, 288):        # lane widths, second column pass, NJ steps, fused limit
        assert edge in ks and edge + 1 in ks
    assert all(rc.sweep_m(K) % 2 == 1 and rc.sweep_m(K) > 2048 for K in ks)
    ms = [m for m, K in rc.GRID_CASES if K == 4]
    assert min(ms) < 65536 < max(ms) and any(m > 2048 * 64 and -(-m // 2048) * 2047 >= m for m in ms)
    assert any(K > 256 and m > 16384 for m, K in rc.GRID_CASES)
    assert any(m > 512 * 4096 for m, _, _ in rc.STATS_CASES)
    assert {n for _, _, n in rc.STATS_CASES} >= {1, 37, rc.STATS_MAX_NCAT}


@pytest.mark.parametrize("args", ALL, ids=ident)
def test_mirror_within_the_bars_and_every_fault_far_outside(args):
    case = rc.make_case(*args)
    ref = rc.reference(case)
    clean = rc.score(case, rc.mirror(case))
    print(f"{case.name}: mirror " + " ".join(f"{k} {v:.3f}" for k, v in clean.items()))
    assert set(clean) == {"aw", "bw", "p", "sse", "s"} and max(clean.values()) <= 1.0, clean
    # bars against the sums of the absolute terms
    assert np.all(ref.p_bar <= 1e-9 * ref.p_terms) and np.all(ref.s_bar <= 1e-9 * ref.s_terms)
    assert ref.sse_bar <= 1e-9 * ref.sse
    assert np.all(ref.p_terms > 0) and np.all(ref.s_terms > 0) and ref.sse > 0
    faults = [f for f in rc.FAULTS if rc.applicable(case, f)]
    assert {"drop_last_row", "drop_block_row", "drop_last_column", "w_for_w2"} <= set(faults)
    assert ("odd_neighbour" in faults) == (case.K % 2 == 1 and case.m > 1)
    assert ("ignore_mask" in faults) == (case.mask is not None and case.m >= 3)
    for f in faults:
        hit = rc.score(case, rc.mirror(case, f))
        print(f"    {f}: " + " ".join(f"{k} {v:.3g}" for k, v in hit.items()))
        assert max(hit.values()) > 100.0, (f, hit)
        # the faults of the sums show in the sums themselves, not only in a neighbouring output
        if f in ("drop_last_row", "drop_block_row", "ignore_mask", "w_for_w2"):
            assert hit["s"] > 100.0, (f, hit)
        if f in ("drop_last_row", "drop_block_row", "ignore_mask"):
            assert hit["sse"] > 100.0, (f, hit)
        if f in ("drop_last_column", "odd_neighbour"):
            assert hit["p"] > 100.0 and hit["aw"] > 100.0, (f, hit)


def test_garbage_rows_differ_from_the_clean_ones_only_in_test_rows():
    case = rc.make_case(rc.GARBAGE_M, 31)
    big, b, w = rc.with_garbage(case)
    t = ~case.mask
    assert t.sum() > 100 and np.isnan(big[t]).all() and np.isposinf(b[t]).all() and np.isneginf(w[t]).all()
    assert rc.same_bits(big[~t], case.big[~t]) and rc.same_bits(b[~t], case.b[~t]) and rc.same_bits(w[~t], case.w[~t])


@pytest.mark.parametrize("args", STATS, ids=ident)
def test_stats_mirror_within_the_bars_and_a_dropped_row_far_outside(args):
    case = rc.make_stats_case(*args)
    ref, bar, terms = rc.stats_reference(case)
    clean = rc.stats_score(case, rc.stats_mirror(case))
    print(f"{case.name}: mirror " + " ".join(f"{v:.3f}" for v in clean))
    assert max(clean) <= 1.0, clean
    assert np.all(bar <= 1e-9 * terms) and np.all(bar[:, :2] == 0)
    if case.ncat >= 4:
        assert not ref[case.empty].any() and ref[case.single, 0] == 1 and ref[case.single, 6] == 0
        assert ref[case.zero_w, 0] >= 2 and ref[case.zero_w, 1] == 0 and not ref[case.zero_w, [3, 7, 8, 9]].any()
    assert np.any((case.cat < 0) | (case.cat >= case.ncat))
    hit = rc.stats_score(case, rc.stats_mirror(case, "drop_category_row"))
    print("    drop_category_row: " + " ".join(f"{v:.3g}" for v in hit))
    assert all(h > 100.0 for h in hit[:1] + hit[2:3] + hit[4:7]), hit
