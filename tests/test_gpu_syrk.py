"""GPU (-m gpu): the statistics kernels 1P, 1A, 1S, 1Q, 1QC, 1T and their reductions through the C ABI against the exact and
long-double references of tests/syrk_cases.py, at geometries forced by the options nblocks, nsplit, short, tiled, quad_min_rows
and fused_pack (the sweeps of syrk_cases.py).  Every geometry runs the `integer` family with np.array_equal and `gauss` and
`uniform` under the a-priori bars gamma_(h+4) x absolute sum, h = syrk_cases.depth of the launch that actually ran; every
launch is held to the kernel and geometry the sweep intends (fsnap_launch_info against the planner rules restated in
syrk_cases.plan).  `pytest -m gpu -s` prints every figure before it is asserted and, at the end of each sweep and of the module,
the worst error / bar per kernel family and statistic (profiles/syrk_accuracy.txt)."""
import numpy as np
import pytest

from fitsnap_amd import _capi

import syrk_cases as sc

pytestmark = pytest.mark.gpu

WORST = {}          # (kernel, family, statistic) -> (error / bar, K, m, options); filled by every case, printed at the end


@pytest.fixture(scope="module")
def ctx():
    c = _capi.HipContext(0)
    yield c
    c.close()
    print_worst()


def print_worst(kernel=None):
    """The worst error / bar met so far per kernel family, input family and statistic, with the case it came from."""
    print("\nworst error / bar per kernel family, input family and statistic: fraction at (K, m, options) | launches")
    for key in sorted(COUNT):
        k, f = key
        if kernel in (None, k):
            print(f"  kernel {k:3s} {f:8s} " + " | ".join(
                "{} {:.3f} at ({}, {}, {})".format(st, *WORST[(k, f, st)]) for st in ("G", "c", "s0", "s1")) + f" | {COUNT[key]} launches")


COUNT = {}


def with_options(ctx, opts, fn):
    """fn() under the options `opts`; every option of the sweeps is back at its default afterwards."""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k, v in sc.OPTION_DEFAULTS.items():
            ctx.set_option(k, v)


def load(ctx, case, lda=0):
    """The rows of `case` onto the context (bound in place with leading dimension lda when given); returns what must stay alive."""
    if not lda:
        ctx.upload_rows(case.A, case.b)
        ctx.set_weights(case.w, case.mask)
        return None
    import torch
    m, K = case.A.shape
    big = np.full((m, lda), 7.0)                 # finite numbers between the rows: a kernel that reads them shows on `integer`
    big[:, 3:3 + K] = case.A
    dev = torch.device("cuda", 0)
    keep = (torch.from_numpy(big).to(dev), torch.from_numpy(case.b).to(dev))
    ctx.bind_rows(keep[0].data_ptr() + 3 * 8, m, K, lda, keep[1].data_ptr())
    ctx.set_weights(case.w, case.mask)
    return keep


def assert_launch(ctx, geo, opts, m=None):
    """The launch the context would make is the one the sweep intends: kernel, and every number of the geometry."""
    info = ctx.launch_info()
    want = sc.plan(geo.m if m is None else m, geo.K, geo.lda or None, num_cu=info["compute_units"], **opts)
    assert sc.family_of(info) == geo.kernel == want["family"], (geo, info)
    for key in ("workgroups", "threads", "chunks_per_wave", "NB", "split", "kernel_or_pairs", "nsplit", "fused_pack"):
        if key in want:
            assert info[key] == want[key], (geo, key, info, want)
    if m is None:
        for key, val in geo.want:
            assert info[key] == val, (geo, key, info)
    return info


def note(kernel, family, res, geo):
    COUNT[(kernel, family)] = COUNT.get((kernel, family), 0) + 1
    for st in ("G", "c", "s0", "s1"):
        key = (kernel, family, st)
        if key not in WORST or res[st] > WORST[key][0]:
            WORST[key] = (res[st], geo.K, geo.m, ",".join(f"{k}={v}" for k, v in geo.opts) or "-")


def run_geo(ctx, geo, seed, families=("integer", "gauss", "uniform")):
    """One geometry: every family through the kernel; `integer` exact, the others under the bars."""
    opts = geo.options()
    entries = sc.sample_entries(geo.K) if geo.K > 512 else None
    for family in families:
        case = sc.make_case(family, geo.m, geo.K, seed)

        def go():
            keep = load(ctx, case, geo.lda)
            info = assert_launch(ctx, geo, opts)
            out = ctx.normal_eq()
            del keep
            return info, out

        info, (G, c, s) = with_options(ctx, opts, go)
        if family == "integer":
            Gr, cr, sr = sc.reference_exact(case)
            bad = [n for n, x, y in (("G", G, Gr), ("c", c, cr), ("s", s, sr)) if not np.array_equal(x, y)]
            print(f"{geo.kernel} K={geo.K} m={geo.m} {dict(geo.opts)} lda={geo.lda or geo.K} integer: "
                  f"{'exact' if not bad else 'DIFFERS in ' + ', '.join(bad)}")
            assert not bad, (geo, bad, int(np.sum(G != Gr)), int(np.sum(c != cr)), s, sr)
            continue
        h = sc.depth(geo.kernel, info, geo.K, geo.m)
        res = sc.check(G, c, s, sc.reference(case, entries), h)
        print(f"{geo.kernel} K={geo.K} m={geo.m} {dict(geo.opts)} lda={geo.lda or geo.K} {family}: h={h} error/bar " +
              " ".join(f"{k}={v:.3g}" for k, v in res.items()))
        note(geo.kernel, family, res, geo)
        assert sc.worst(res) <= 1.0, (geo, family, h, res)
        if family == "typed":
            assert G[0, 1] == 0.0 and G[1, 0] == 0.0         # offset columns of disjoint supports: not one rounding between them


def parts(kernel, budget=2.5e8):
    """(K, first, last) slices of a kernel's sweep whose long-double references cost about `budget` multiplications each."""
    fn, Ks = sc.SWEEPS[kernel]
    out = []
    for K in Ks:
        geos = fn(K)
        i0, cost = 0, 0.0
        for i, g in enumerate(geos):
            cost += g.m * (min(K, 512) ** 2 if K <= 512 else 60000)
            if cost > budget or i == len(geos) - 1:
                out.append(pytest.param(K, i0, i + 1, id=f"K{K}-{i0}:{i + 1}"))
                i0, cost = i + 1, 0.0
    return out


def run_part(ctx, kernel, K, i0, i1):
    fn, Ks = sc.SWEEPS[kernel]
    for i, geo in enumerate(fn(K)[i0:i1]):
        run_geo(ctx, geo, seed=1000 + i0 + i)
    if K == Ks[-1] and i1 == len(fn(K)):          # the sweep's last part: its summary
        print_worst(kernel)


@pytest.mark.parametrize("K,i0,i1", parts("1A"))
def test_kernel_1a_chunks_per_wave_trips_and_row_waves(ctx, K, i0, i1):
    # 1 ... 14 chunks per wave in one workgroup (ragged last chunk, shorter and empty last waves), 12 ... 18 on 2, 3 and 17
    # workgroups (the ring's period six, full and half trips), pairs packed in LDS and read from HBM, and beyond the LDS
    run_part(ctx, "1A", K, i0, i1)


@pytest.mark.parametrize("K,i0,i1", parts("1P"))
def test_kernel_1p_chunks_per_wave_and_strided_rows(ctx, K, i0, i1):
    # 1 ... 20 and 31 ... 33 chunks per wave (rings of 6 and 8 slots), both packings, odd K on an odd leading dimension
    run_part(ctx, "1P", K, i0, i1)


@pytest.mark.parametrize("K,i0,i1", parts("1S"))
def test_kernel_1s_chunk_lengths_and_phases(ctx, K, i0, i1):
    # chunks of 32 rows, of one, two and three phases +- 4 rows, on 1 ... 17 chunks (8 = one grid row of workgroups); pairs from HBM
    run_part(ctx, "1S", K, i0, i1)


@pytest.mark.parametrize("K,i0,i1", parts("1Q"))
def test_kernel_1q_trips_per_workgroup(ctx, K, i0, i1):
    run_part(ctx, "1Q", K, i0, i1)


@pytest.mark.parametrize("K,i0,i1", parts("1QC"))
def test_kernel_1qc_clusters(ctx, K, i0, i1):
    run_part(ctx, "1QC", K, i0, i1)


@pytest.mark.parametrize("K,i0,i1", parts("1T"))
def test_kernel_1t_splits_and_both_reductions(ctx, K, i0, i1):
    # 1, 2, 7, 16 splits on fsnap_reduce_tiled_small, 17 and 33 on fsnap_reduce_tiled
    run_part(ctx, "1T", K, i0, i1)


TYPED = [sc._geo("1P", 33, 16 * 2 * 17 - 3, nblocks=2), sc._geo("1A", 142, 16 * 3 * 13 - 1, short=0, nblocks=3),
         sc._geo("1S", 142, 3 * 116 - 1, nblocks=3), sc._geo("1Q", 168, 4 * 2 * 25 - 1, quad_min_rows=0, nblocks=2),
         sc._geo("1QC", 304, 4 * 2 * 25 - 3, quad_min_rows=0, nblocks=4), sc._geo("1T", 193, 16 * 2 * 9 - 1, tiled=1, nsplit=2)]


@pytest.mark.parametrize("geo", TYPED, ids=[g.kernel for g in TYPED])
def test_typed_rows_keep_exact_zeros_between_offset_columns(ctx, geo):
    run_geo(ctx, geo, seed=77, families=("typed",))


REDUCE = [pytest.param(kern, K, nb, id=f"{kern}-K{K}-np{nb}") for kern, Ks in sc.K_REDUCE.items() for K in Ks
          for nb in sc.NP_REDUCE if not (kern == "1A" and nb > 257)]


@pytest.mark.parametrize("kernel,K,nb", REDUCE)
def test_reduction_partial_counts_plain_and_accumulating(ctx, kernel, K, nb):
    # kernel 2b's batch of 16 loads per slice (p + 240 < np) against its tail, slice by slice: np around 16, 32, 240, 256, 272
    # and 512; the c region of kernel 1P and 1A has 4 np partials.  Then the same launch adding to a buffer that already holds
    # the statistics of a second batch of another geometry: on `integer` the total is the one-shot statistics exactly.
    import torch
    geo, m2 = next(x for x in sc.sweep_reduce(kernel, K) if x[0].want == (("workgroups", nb),))
    opts, opts2 = geo.options(), sc.second_batch_opts(kernel)
    for family in ("integer", "gauss", "uniform"):
        first, second = sc.make_case(family, geo.m, K, nb), sc.make_case(family, m2, K, 5000 + nb)
        total = torch.zeros(K * K + K + 3, dtype=torch.float64, device=torch.device("cuda", 0))

        def batch2():
            load(ctx, second)
            info = ctx.launch_info()
            ctx.normal_eq_accumulate(total.data_ptr())
            return info

        def batch1():
            load(ctx, first)
            info = assert_launch(ctx, geo, opts)
            plain = ctx.normal_eq()
            ctx.normal_eq_accumulate(total.data_ptr())
            return info, plain

        info2 = with_options(ctx, opts2, batch2)
        info1, plain = with_options(ctx, opts, batch1)
        assert (info1["workgroups"], info1["chunks_per_wave"]) != (info2["workgroups"], info2["chunks_per_wave"])
        both = ctx.download_packed(total.data_ptr(), K)
        if family == "integer":
            one, two = sc.reference_exact(first), sc.reference_exact(second)
            assert all(np.array_equal(x, y) for x, y in zip(plain, one)), (geo, "plain")
            assert all(np.array_equal(x, y + z) for x, y, z in zip(both, one, two)), (geo, "accumulate")
            continue
        ref1 = sc.reference(first)
        h1 = sc.depth(kernel, info1, K, geo.m)
        h2 = sc.depth(sc.family_of(info2), info2, K, m2, accumulate=True)
        for what, (G, c, s), ref, h in (("plain", plain, ref1, h1),
                                        ("accumulate", both, sc.add_refs(ref1, sc.reference(second)), {k: max(h1[k] + 1, h2[k]) for k in h1})):
            res = sc.check(G, c, s, ref, h)
            print(f"{kernel} K={K} m={geo.m} np={nb} {what} {family}: h={h} error/bar " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
            note(kernel, family, res, geo)
            assert sc.worst(res) <= 1.0, (geo, what, family, h, res)


EXACT = [sc._geo("1P", 33, 16 * 2 * 17 - 3, nblocks=2), sc._geo("1P", 64, 16 * 2 * 17 - 3, nblocks=2),
         sc._geo("1A", 129, 16 * 3 * 13 - 1, short=0, nblocks=3), sc._geo("1A", 128, 16 * 3 * 13 - 1, short=0, nblocks=3),
         sc._geo("1S", 142, 3 * 116 - 1, nblocks=3), sc._geo("1S", 96, 3 * 132 - 1, nblocks=3),
         sc._geo("1Q", 168, 4 * 2 * 25 - 1, quad_min_rows=0, nblocks=2), sc._geo("1Q", 180, 4 * 2 * 25 - 1, quad_min_rows=0, nblocks=2),
         sc._geo("1QC", 304, 4 * 2 * 25 - 3, quad_min_rows=0, nblocks=4), sc._geo("1QC", 384, 4 * 2 * 25 - 3, quad_min_rows=0, nblocks=8),
         sc._geo("1T", 193, 16 * 2 * 9 - 1, tiled=1, nsplit=2), sc._geo("1T", 256, 16 * 2 * 9 - 1, tiled=1, nsplit=2)]


@pytest.mark.parametrize("geo", EXACT, ids=[f"{g.kernel}-K{g.K}" for g in EXACT])
def test_exact_properties_on_one_launch_geometry(ctx, geo):
    # scalings by powers of two commute with every rounding, and a row that must not count leaves the same bits however it is
    # taken out -- once per kernel family at an odd and an even number of 16-column blocks, all on one launch geometry
    base = sc.make_case("uniform", geo.m, geo.K, 9)
    opts = geo.options()
    K, m = geo.K, geo.m

    def stats(A, b, w, testing):
        case = sc.Case("uniform", np.ascontiguousarray(A), b, w, testing)

        def go():
            load(ctx, case)
            assert_launch(ctx, geo, opts)
            return ctx.normal_eq()

        return with_options(ctx, opts, go)

    A, b, w, t = base.A, base.b, base.w, base.testing
    G, c, s = stats(A, b, w, t)
    assert np.array_equal(G, G.T)
    G1, c1, s1 = stats(A, b, w, t)                                   # run to run
    assert np.array_equal(G, G1) and np.array_equal(c, c1) and np.array_equal(s, s1)
    G2, c2, s2 = stats(A, b, 2.0 * w, t)                             # weights x 2
    assert np.array_equal(G2, 4.0 * G) and np.array_equal(c2, 4.0 * c) and s2[0] == 4.0 * s[0] and s2[1] == 2.0 * s[1]
    for j in (K - 1, K // 2):                                        # one column x 2^5
        A3 = A.copy()
        A3[:, j] *= 32.0
        G3, c3, s3 = stats(A3, b, w, t)
        Ge, ce = G.copy(), c.copy()
        Ge[j, :] *= 32.0
        Ge[:, j] *= 32.0
        ce[j] *= 32.0
        assert np.array_equal(G3, Ge) and np.array_equal(c3, ce) and np.array_equal(s3, s)
    G4, c4, s4 = stats(A, 2.0 * b, w, t)                             # b x 2
    assert np.array_equal(G4, G) and np.array_equal(c4, 2.0 * c) and s4[0] == 4.0 * s[0] and s4[1] == 2.0 * s[1]
    for r in (m // 2 | 1, m - 1, 0):                                 # a testing row = the row at weight 0 = zeros at weight 1
        At, tt = A.copy(), t.copy()
        At[r] = np.nan
        tt[r] = True
        Az, wz = A.copy(), w.copy()
        Az[r] = np.inf
        wz[r] = 0.0
        A0, b0, w0 = A.copy(), b.copy(), w.copy()
        A0[r] = 0.0
        b0[r] = 0.0
        w0[r] = 1.0
        (Ga, ca, sa), (Gb, cb, sb), (Gc, cc, sc_) = stats(At, b, w, tt), stats(Az, b, wz, t), stats(A0, b0, w0, t)
        assert np.array_equal(Ga, Gb) and np.array_equal(Ga, Gc) and np.array_equal(ca, cb) and np.array_equal(ca, cc)
        assert np.array_equal(sa[:2], sb[:2]) and np.array_equal(sa[:2], sc_[:2])
        assert sa[2] == m - 1 and sb[2] == m and sc_[2] == m
        assert not np.array_equal(Ga, G)
