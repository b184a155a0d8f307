"""CPU: the float64 mirror of tests/syrk_cases.py at the geometries of the GPU sweeps (tests/test_gpu_syrk.py), computed by the
restated planner rules for 256 CUs -- `integer` gives the exact bits, the other families sit inside the a-priori bars, depth() is
not below the counted height, the long-double reference's own error is below 1/100 of every bar -- and the thirteen switchable
faults against the same checks.  The K lists are thinned (both parities of the block count and a partial last block stay);
the geometries are all there."""
import math

import numpy as np
import pytest

import syrk_cases as sc

K_CPU = {"1A": (113, 144), "1P": (1, 17, 33, 80), "1S": (110, 142), "1Q": (150, 264), "1QC": (304, 384), "1T": (31, 193, 513)}
K_REDUCE_CPU = {"1P": 16, "1A": 96}


def exact(mir, case):
    Gr, cr, sr = sc.reference_exact(case)
    return np.array_equal(mir.G, Gr) and np.array_equal(mir.c, cr) and np.array_equal(mir.s, sr)


def hold(geo, info, seed, families, prev_of=None):
    """The mirror of one geometry on every family; returns the worst error / bar met."""
    h = sc.depth(geo.kernel, info, geo.K, geo.m)
    entries = sc.sample_entries(geo.K) if geo.K > 512 else None
    top = 0.0
    for family in families:
        case = sc.make_case(family, geo.m, geo.K, seed)
        mir = sc.mirror(case, geo.kernel, info, geo.K)
        assert all(h[k] >= mir.h[k] for k in h), (geo, h, mir.h)
        if family == "integer":
            assert exact(mir, case), geo
            continue
        ref = sc.reference(case, entries)
        assert sc.ref_uncertainty_over_bar(ref, h) < 0.01, (geo, ref.unc, h)
        res = sc.check(mir.G, mir.c, mir.s, ref, h)
        assert sc.worst(res) <= 1.0, (geo, family, res)
        top = max(top, sc.worst(res))
    return top


@pytest.mark.parametrize("kernel,K", [(k, K) for k, Ks in K_CPU.items() for K in Ks])
def test_mirror_exact_on_integer_and_inside_the_bars_at_every_sweep_geometry(kernel, K):
    geos = sc.SWEEPS[kernel][0](K)
    top = 0.0
    for i, geo in enumerate(geos):
        families = ("integer", "gauss", "uniform") + (("typed",) if K >= 3 and i % 4 == 0 else ())
        top = max(top, hold(geo, geo.info(), 1000 + i, families))
    print(f"kernel {kernel} K={K}: {len(geos)} geometries, worst mirror error / bar {top:.3f}")
    assert 0.0 < top <= 1.0


@pytest.mark.parametrize("kernel", list(K_REDUCE_CPU))
def test_mirror_at_every_partial_count_plain_and_accumulating(kernel):
    K = K_REDUCE_CPU[kernel]
    for geo, m2 in sc.sweep_reduce(kernel, K):
        info = geo.info()
        nb = info["workgroups"]
        hold(geo, info, nb, ("integer", "uniform"))
        for family in ("integer", "gauss"):
            whole = sc.make_case(family, geo.m + m2, K, 5000 + nb)
            first = sc.Case(family, whole.A[:geo.m], whole.b[:geo.m], whole.w[:geo.m], whole.testing[:geo.m])
            second = sc.Case(family, whole.A[geo.m:], whole.b[geo.m:], whole.w[geo.m:], whole.testing[geo.m:])
            info2 = sc.plan(m2, K, **sc.second_batch_opts(kernel))
            m2nd = sc.mirror(second, info2["family"], info2, K, prev=(np.zeros((K, K)), np.zeros(K), np.zeros(3)))
            mir = sc.mirror(first, kernel, info, K, prev=(m2nd.G, m2nd.c, m2nd.s))
            h1, h2 = sc.depth(kernel, info, K, geo.m, accumulate=True), sc.depth(info2["family"], info2, K, m2, accumulate=True)
            h = {k: max(h1[k], h2[k]) for k in h1}
            assert all(h1[k] >= mir.h[k] for k in h), (geo, h1, mir.h)
            if family == "integer":
                assert exact(mir, whole), geo
            else:
                ref = sc.add_refs(sc.reference(first), sc.reference(second))
                assert sc.ref_uncertainty_over_bar(ref, h) < 0.01
                assert sc.worst(sc.check(mir.G, mir.c, mir.s, ref, h)) <= 1.0, geo


# (fault, sweep) pairs in which the fault cannot change a single bit at any geometry of the sweep, and why
NO_HALF_TRIP = "the kernel's loop has no half trip (rings of compile-time slots, or staged phases)"
NO_241 = "no region of the sweep's launches has 241 ... 255 partials"
ROWS_4 = "every row count of the sweep is a multiple of four"
NO_ACC = "the sweep has no accumulating launch (the reduction sweeps have)"
NOT_ACTING = {
    (3, "1P"): NO_HALF_TRIP, (3, "1S"): NO_HALF_TRIP, (3, "1T"): NO_HALF_TRIP, (3, "reduce-1P"): NO_HALF_TRIP,
    (6, "1T"): "64-column superblocks are four interleaved blocks: there is no plain last block",
    (9, "1A"): NO_241, (9, "1P"): NO_241, (9, "1S"): NO_241, (9, "1Q"): NO_241, (9, "1QC"): NO_241,
    (9, "1T"): "the tiled reductions have no batch of 16 loads per slice",
    (1, "reduce-1P"): ROWS_4, (1, "reduce-1A"): ROWS_4,
    (6, "reduce-1A"): "96 columns are six blocks (the GPU run has 142 as well)",
    (7, "reduce-1P"): "16 columns are one tile",
    (11, "1A"): NO_ACC, (11, "1P"): NO_ACC, (11, "1S"): NO_ACC, (11, "1Q"): NO_ACC, (11, "1QC"): NO_ACC, (11, "1T"): NO_ACC,
}
FAULT_SWEEPS = list(K_CPU) + ["reduce-" + k for k in K_REDUCE_CPU]


def sweep_geos(sweep):
    """(geometry, rows of an accumulating second batch or 0) of a sweep at the CPU run's K list."""
    if sweep.startswith("reduce-"):
        kernel = sweep[7:]
        return [(g, m2) for g, m2 in sc.sweep_reduce(kernel, K_REDUCE_CPU[kernel]) if g.m <= 20000 or g.info()["workgroups"] in (241, 255, 257)]
    return [(g, 0) for K in K_CPU[sweep] if K <= 512 for g in sc.SWEEPS[sweep][0](K)]


def detect(geo, info, fault, m2, seed):
    """(integer sees it, worst bars outside on gauss, on uniform) for one fault at one geometry."""
    out = []
    for family in ("integer", "gauss", "uniform"):
        case = sc.make_case(family, geo.m + m2, geo.K, seed)
        prev = None
        if m2:
            second = sc.Case(family, case.A[geo.m:], case.b[geo.m:], case.w[geo.m:], case.testing[geo.m:])
            info2 = sc.plan(m2, geo.K, **sc.second_batch_opts(geo.kernel))
            m2nd = sc.mirror(second, info2["family"], info2, geo.K, prev=(np.zeros((geo.K, geo.K)), np.zeros(geo.K), np.zeros(3)))
            prev = (m2nd.G, m2nd.c, m2nd.s)
            first = sc.Case(family, case.A[:geo.m], case.b[:geo.m], case.w[:geo.m], case.testing[:geo.m])
        else:
            first = case
        mir = sc.mirror(first, geo.kernel, info, geo.K, faults=(fault,), prev=prev)
        if family == "integer":
            out.append(not exact(mir, case))
        else:
            h = sc.depth(geo.kernel, info, geo.K, geo.m, accumulate=bool(m2))
            ref = sc.reference(case)
            out.append(sc.worst(sc.check(mir.G, mir.c, mir.s, ref, h)))
    return out


@pytest.mark.parametrize("fault", sorted(sc.FAULTS))
@pytest.mark.parametrize("sweep", FAULT_SWEEPS)
def test_every_fault_is_caught_wherever_it_can_act(sweep, fault):
    acting = []
    for geo, m2 in sweep_geos(sweep):
        info = geo.info()
        for acc in ((False, True) if m2 else (False,)):
            case = sc.make_case("integer", geo.m + (m2 if acc else 0), geo.K, 31)
            head = sc.Case("integer", case.A[:geo.m], case.b[:geo.m], case.w[:geo.m], case.testing[:geo.m])
            if sc.can_act(fault, geo, info, head, accumulate=acc):
                acting.append((geo, info, m2 if acc else 0))
    if not acting:
        assert (fault, sweep) in NOT_ACTING, (fault, sc.FAULTS[fault], sweep)
        return
    assert (fault, sweep) not in NOT_ACTING
    acting.sort(key=lambda x: x[0].m * x[0].K)
    picks = {0, len(acting) // 3, len(acting) // 2, (2 * len(acting)) // 3}          # small and middling geometries
    for i in sorted(picks):
        geo, info, m2 = acting[i]
        seen, gauss, uniform = detect(geo, info, fault, m2, 31)
        print(f"fault {fault:2d} {sweep} K={geo.K} m={geo.m} {dict(geo.opts)}: integer {'differs' if seen else 'equal'}, "
              f"gauss {gauss:.3g} bars, uniform {uniform:.3g} bars")
        assert seen or gauss > 100.0 or uniform > 100.0, (fault, sc.FAULTS[fault], geo)
        if fault == 12:
            # a loss of precision: every integer x is a float32 number too -- only the bars can see it
            assert not seen and gauss > 100.0 and uniform > 100.0, geo
        if fault == 13:
            assert gauss > 100.0 or uniform > 100.0, geo
            # the partial sums of {4, 1, 2^-10}-weighted integers need more than 24 bits; with unit weights they do not, and the
            # rounded partial is the same number
            unit = sc.make_case("integer", geo.m, geo.K, 31, weights=(1.0,))
            assert exact(sc.mirror(unit, geo.kernel, info, geo.K, faults=(13,)), unit), geo


def test_planner_restatement_examples():
    # shapes whose geometry the GPU suite asserts through fsnap_launch_info (tests/test_gpu_short.py, tests/test_gpu_parity.py)
    assert sc.plan(13035, 142)["family"] == "1S" and sc.plan(13035, 142)["threads"] == 512
    assert sc.plan(40003, 142, short=1)["chunks_per_wave"] > 128
    assert sc.plan(100003, 110)["family"] == "1A"
    assert sc.plan(1000000, 128)["family"] == "1A" and sc.plan(1000000, 128)["workgroups"] == 256
    assert sc.plan(30011, 176)["family"] == "1Q"
    assert math.isclose(sc.gamma(10), 10 * 2.0 ** -53, rel_tol=1e-12)
