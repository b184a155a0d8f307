"""Inputs, references, a-priori bars and a float64 mirror for the statistics kernels:
kernel 1P `fsnap_syrk_wave_p`, 1A `fsnap_syrk_acc`, 1T `fsnap_syrk_tiled` (fsnap_syrk.hip), 1S `fsnap_syrk_short`
(fsnap_syrk_short.hip), 1Q / 1QC `fsnap_syrk_quad` / `fsnap_syrk_quadc` (fsnap_syrk_quad.hip) and the reductions
`fsnap_reduce_partials2`, `fsnap_reduce_tiled`, `fsnap_reduce_tiled_small`.  Used by tests/test_syrk_cases_cpu.py (no GPU:
the mirror against the bars, the faults against both) and tests/test_gpu_syrk.py (the kernels against the same bars).

Input families (`make_case`), all seeded and small
  integer  A in -3 ... 3 times a power of two per column, b in -3 ... 3, weights from {4, 1, 2^-10}, 20 % testing rows filled with
           NaN / Inf in A, b and w, 5 % zero-weight rows whose A is Inf.  Every product w^2 a_i a_j is an integer multiple of
           2^-20 2^(s_i + s_j) below 144 2^(s_i + s_j), so with m 144 2^20 < 2^53 every partial sum in ANY order is exact: the
           statistics are the same bits on every kernel and geometry, the reference is the float64 product of the cleaned rows
           and the comparison is np.array_equal.  One dropped, doubled, misplaced or leaked row, column or partial shows at one
           unit whatever its weight.
  gauss    the distribution of tests/test_gpu_parity.py: columns scaled by 10^U(-3, 3), weights {100, 1, 1e-8}, 20 % testing rows.
  uniform  Gaussian rows, weights U(0.5, 2), no testing rows: every row is visible at the bar.
  typed    FitSNAP-like rows: a few energy rows of magnitude 1e2 with one 0/1 offset column per type, many force rows of 1e-1
           and some stress rows with zeros in the offset columns.  The offset columns have disjoint supports: G_01 is exactly 0.
Integer data cannot see a loss of precision (fault 12: every x is a float32 number as well); the Gaussian families cannot see a
fault confined to invisible rows (a 1e-8-weight row is 1e-16 of an entry).  Both kinds are needed.

Reference of the non-integer families (`reference`): x = w_eff a in long double (64-bit significand: the product of two
doubles rounds at 2^-64), G = x^T x, c = x^T (w b), sum (w b)^2, sum w b in long double in blocks of max(64, sqrt(m)) rows, with the absolute
sums S_ij = sum |x_ri x_rj|, T_j = sum |x_rj w_r b_r|, sum (w b)^2, sum |w b| beside them.  Its own error is at most
(block + blocks + 3) 2^-64 of the absolute sum (`Ref.unc`), below 1/100 of every bar here (asserted on the CPU).  For K > 512 the
long-double entries are a sample: the diagonal, the last 16-column block row and column, all of c, and 4096 further entries.

Bars (`check`): a summation tree in which no term passes through more than h additions gives
    |G^_ij - G_ij| <= gamma_(h+4) S_ij,      gamma_n = n eps / (1 - n eps), eps = 2^-53
and likewise c against T_j, sum (w b)^2 against itself, sum w b against sum |w b|; the + 4 is the rounding of w_eff a on both
sides, the product, and kernel 1T's w^2 a_I.  n_train is exact, G == G.T bitwise.

h per kernel (`depth`), read from the code -- never fitted to what a GPU returns.  One v_mfma_f64_16x16x4_f64 counts as four
additions (its four row products are added to the accumulator in an order the ISA does not state).
  1A  fsnap_syrk.hip:470-483 one accumulator chain per row-wave over its chunks_per_wave chunks: 4 cpw; :524-525 the four
      row-waves ((s0 + s1) + s2) + s3: 3; then kernel 2b over np = workgroups partials.  c: one FMA per chunk and lane (:337,
      :455): cpw; xlane_sum_rows :67-72: 2; np = 4 workgroups.  Scalars with fused packing, pack_rows_to_lds :281-318: a lane
      takes every 64th row of the wave: ceil(4 cpw / 64), a butterfly of 6; np = 4 workgroups.
  1P  :638-665 the same chain, 4 cpw; the fold {2, 3} -> {0, 1}, 1 -> 0 (:671-699): 2.  c and the scalars as kernel 1A.
  1S  fsnap_syrk_short.hip:315-327 a tile's chain runs over all rows of its chunk, phase after phase, in whole pairs of 4-row
      steps (:241): sum of ((nr + 7) & ~7) over the phases; no fold; np = chunks.  c: thread (rg, u) takes every RG-th row
      of a phase (:268-300), RG = 512 / (8 NB): ceil(RP / RG) per phase; the RG row groups in order (:381-383): RG - 1.
      Scalars: one row per phase and thread (:243-256), a butterfly of 6, wave 0 + wave 1 (:396): phases + 7.
  1Q / 1QC  fsnap_syrk_quad.hip:443-463 every tile has one owner wave whose chain runs over the workgroup's (cluster's)
      chunks: 4 cpg; no fold (:493-499); np = workgroups (clusters).  c: cpg + 2 (:503-509), np = 4 C per workgroup with
      zeros from the waves that do not own the block.  Scalars (:546-578): thread t takes rows t, t + 256, ...: ceil(4 cpg / 256),
      a butterfly of 6.
  1T  fsnap_syrk.hip:976-997 a wave's chain over a quarter of the split's chunks: 4 (cps / 4); fold :1042-1071: 2; the splits
      in order (fsnap_reduce_tiled_small :1184, at most 16) or sliced (fsnap_reduce_tiled :1228-1244: ceil(np / 16) + 2 + 16).
      c: cps / 4 + 2, then np = 4 nsplit partials, slice g takes g, g + 16, ... (:1223-1226) and the 16 slices.
  2b  fsnap_reduce_partials2 :744-770: slice s of 16 takes partials s, s + 16, ...: at most ceil(np / 16) additions in one of
      four interleaved accumulators, (a0 + a1) + (a2 + a3): 2, the 16 slices in order: 16.
  packing kernel (fused_pack = 0, kernel 1T always) fsnap_rows.hip:516-539: a thread takes every (256 blocks)-th row,
      a tree of 8; np = pack_weights_num_blocks(m) partials.
  accumulate: one more addition (the total so far + this batch).

Mirror (`mirror`): float64 numpy in exactly these trees -- chunk -> chain per row-wave, tile owner or member -> fold -> partials in
the order of kernel 2b or of the tiled reductions, in the even/odd column interleave of the kernels (col_of) with the scatter
that undoes it and mirrors the triangle, kernel 1T's (w^2 a_I) a_J off the diagonal superblocks, and the accumulate flag.  It
counts the additions every term passes through (`Mirror.h`), so `depth` can be held against it; it does not reproduce the
GPU's bits (no FMA, the MFMA's inner order is unknown).  `FAULTS` names thirteen switchable defects a statistics kernel could
really have; tests/test_syrk_cases_cpu.py shows that the families and bars catch each one wherever it can act.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

EPS = 2.0 ** -53
NUM_CU = 256                      # MI355X
LD = np.longdouble

FAULTS = {
    1: "the ragged tail rows of the last chunk are dropped",
    2: "a row-wave's clipped range runs one chunk into its neighbour's",
    3: "the half trip skips the last of 1 ... 3 leftover chunks",
    4: "a masked row enters with its w instead of 0",
    5: "a zero-weight row's Inf is fetched",
    6: "the interleave is not undone for an odd last block",
    7: "an off-diagonal tile is mirrored to the wrong transpose position",
    8: "the reduction's scalar tail omits a partial when np = 1 (mod 16)",
    9: "the batch loop's last slices omit theirs for 240 < np < 256",
    10: "c takes w b of the neighbouring row of its chunk",
    11: "the accumulate flag is ignored in the c region",
    12: "x is rounded to float32 in one column block",
    13: "one workgroup's partial is rounded to float32 before the reduction",
}


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


# ---------------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    family: str
    A: np.ndarray
    b: np.ndarray
    w: np.ndarray
    testing: np.ndarray            # bool, True = testing row (mask 0)

    @property
    def mask(self):
        return (~self.testing).astype(np.uint8)

    def clean(self):
        """(x, wb, keep) of the rows as the statistics see them, float64: x = w_eff a, wb = w_eff b, 0 where w_eff == 0."""
        keep = ~self.testing
        w_eff = np.where(keep, self.w, 0.0)
        live = w_eff != 0.0
        a = np.where(live[:, None], self.A, 0.0)
        bb = np.where(keep, self.b, 0.0)
        return w_eff[:, None] * a, w_eff * bb, keep


def make_case(family, m, K, seed, weights=None):
    """One seeded input of `family`; `weights` replaces the integer family's weight set."""
    rng = np.random.default_rng([seed, m, K, sorted(("integer", "gauss", "uniform", "typed")).index(family)])
    if family == "integer":
        assert m * 144 * 2 ** 20 < 2 ** 53
        A = rng.integers(-3, 4, size=(m, K)).astype(np.float64) * 2.0 ** rng.integers(-2, 3, size=K)
        b = rng.integers(-3, 4, size=m).astype(np.float64)
        w = rng.choice(np.asarray(weights if weights is not None else (4.0, 1.0, 2.0 ** -10)), size=m)
        t = rng.random(m) < 0.2
        z = (rng.random(m) < 0.05) & ~t
        A[t] = np.where(rng.random((int(t.sum()), K)) < 0.5, np.nan, np.inf)
        b[t] = np.inf
        w[t] = np.where(rng.random(int(t.sum())) < 0.5, np.nan, -np.inf)
        w[z] = 0.0                 # (b stays finite there: 0 * Inf is NaN in the reference's w * b as well)
        A[z] = np.inf
    elif family == "gauss":
        A = rng.standard_normal((m, K)) * (10.0 ** rng.uniform(-3, 3, size=K))
        b = rng.standard_normal(m)
        w = rng.choice([100.0, 1.0, 1e-8], size=m, p=[0.03, 0.83, 0.14])
        t = rng.random(m) < 0.2
        A[t] = np.nan
        b[t] = np.inf
        w[t] = -np.inf
    elif family == "uniform":
        A = rng.standard_normal((m, K))
        b = rng.standard_normal(m)
        w = rng.uniform(0.5, 2.0, size=m)
        t = np.zeros(m, dtype=bool)
    elif family == "typed":
        assert K >= 3
        kind = rng.choice(3, size=m, p=[0.05, 0.85, 0.10])           # energy, force, stress
        A = rng.standard_normal((m, K)) * np.asarray([1e2, 1e-1, 1.0])[kind][:, None]
        A[:, :2] = 0.0
        en = np.flatnonzero(kind == 0)
        A[en, rng.integers(0, 2, size=en.size)] = 1.0                # one offset column per energy row: disjoint supports
        b = rng.standard_normal(m) * np.asarray([1e2, 1e-1, 1.0])[kind]
        w = np.asarray([100.0, 1.0, 1e-2])[kind]
        t = rng.random(m) < 0.1
    else:
        raise ValueError(family)
    return Case(family, np.ascontiguousarray(A), b, w, t)


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    G: np.ndarray                  # (K, K), or (n,) at `entries`
    c: np.ndarray
    s: np.ndarray                  # [sum (w b)^2, sum w b, n_train]
    S: np.ndarray                  # absolute sums in the shape of G
    T: np.ndarray
    s_abs: np.ndarray              # [sum (w b)^2, sum |w b|]
    unc: float                     # the reference's own error as a multiple of 2^-64 of the absolute sums
    entries: tuple | None = None   # (rows, cols) of a sampled G


def reference_exact(case):
    """The integer family: float64, exact in any order."""
    x, wb, keep = case.clean()
    return x.T @ x, x.T @ wb, np.asarray([wb @ wb, wb.sum(), float(keep.sum())])


def sample_entries(K, seed=0):
    rng = np.random.default_rng([seed, K])
    d = np.arange(K)
    lo = 16 * ((K - 1) // 16)
    last = np.arange(lo, K)
    rr = [d, np.repeat(last, K), np.tile(d, last.size), rng.integers(0, K, 4096)]
    cc = [d, np.tile(d, last.size), np.repeat(last, K), rng.integers(0, K, 4096)]
    return np.concatenate(rr), np.concatenate(cc)


def _sampled(x, K):
    """sum_r x_ri x_rj at the entries of sample_entries(K), in their order, without gathering the dense parts."""
    lo = 16 * ((K - 1) // 16)
    rnd = sample_entries(K)
    rnd = (rnd[0][-4096:], rnd[1][-4096:])
    last = (x[:, lo:].T @ x).ravel()
    return np.concatenate([np.einsum("ri,ri->i", x, x), last, last, np.einsum("ri,ri->i", x[:, rnd[0]], x[:, rnd[1]])])


def reference(case, entries=None):
    """Long-double statistics and their absolute sums (module docstring); `entries` = (rows, cols) samples G."""
    keep = ~case.testing
    w_eff = np.where(keep, case.w, 0.0)
    live = w_eff != 0.0
    xl = w_eff.astype(LD)[:, None] * np.where(live[:, None], case.A, 0.0).astype(LD)
    wbl = w_eff.astype(LD) * np.where(keep, case.b, 0.0).astype(LD)
    m, K = xl.shape
    block = max(64, math.isqrt(m))
    G = np.zeros((K, K) if entries is None else len(entries[0]), LD)
    c = np.zeros(K, LD)
    s0 = s1 = LD(0)
    nblk = 0
    for r0 in range(0, m, block):
        xb, wb = xl[r0:r0 + block], wbl[r0:r0 + block]
        if entries is None:
            for i0 in range(0, K, 64):                       # the upper triangle in panels of 64 rows of G
                G[i0:i0 + 64, i0:] += xb[:, i0:i0 + 64].T @ xb[:, i0:]
        else:
            G += _sampled(xb, K)
        c += xb.T @ wb
        s0 += wb @ wb
        s1 += wb.sum()
        nblk += 1
    if entries is None:
        G = np.triu(G) + np.triu(G, 1).T
    x = np.abs(np.asarray(xl, dtype=np.float64))
    wb = np.abs(np.asarray(wbl, dtype=np.float64))
    S = x.T @ x if entries is None else _sampled(x, K)
    s = np.asarray([s0, s1, LD(int(keep.sum()))])
    return Ref(G, c, s, S, x.T @ wb, np.asarray([wb @ wb, wb.sum()]), float(min(block, m) + nblk + 3), entries)


def add_refs(r1, r2):
    """Reference of two batches accumulated into one buffer."""
    return Ref(r1.G + r2.G, r1.c + r2.c, r1.s + r2.s, r1.S + r2.S, r1.T + r2.T, r1.s_abs + r2.s_abs, max(r1.unc, r2.unc) + 1,
               r1.entries)


def ref_uncertainty_over_bar(ref, h):
    """The reference's own error bound over the smallest bar of the heights h (both are multiples of the same absolute sums)."""
    return ref.unc * 2.0 ** -64 / gamma(min(h.values()) + 4)


def _ratio(err, bar):
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)         # a zero bar admits a zero error only
    return r


def check(G, c, s, ref, h):
    """Worst error / bar of G, c, sum (w b)^2 and sum w b against `ref` for the heights h = depth(...); NaN counts as inf.
    Returns {"G": ratio, "c": ..., "s0": ..., "s1": ..., "n": 0 or inf, "sym": 0 or inf}."""
    Gs = G if ref.entries is None else G[ref.entries[0], ref.entries[1]]
    out = {}
    for name, got, want, scale, hh in (("G", Gs, ref.G, ref.S, h["G"]), ("c", c, ref.c, ref.T, h["c"]),
                                        ("s0", s[0], ref.s[0], ref.s_abs[0], h["s"]), ("s1", s[1], ref.s[1], ref.s_abs[1], h["s"])):
        err = np.abs(np.asarray(got, dtype=LD) - want)
        r = _ratio(err, gamma(hh + 4) * np.asarray(scale))
        r = np.where(np.isnan(r), np.inf, r)
        out[name] = float(np.max(r))
    out["n"] = 0.0 if float(s[2]) == float(ref.s[2]) else math.inf
    out["sym"] = 0.0 if np.array_equal(G, G.T) else math.inf
    return out


def worst(res):
    return max(res.values())


# ---------------------------------------------------------------------------------------------------------------------------
# the planner's rules (fsnap_capi.cpp: plan_geometry, quad_chunks_per_wg, tiled_geometry) for one device of `num_cu` CUs
# ---------------------------------------------------------------------------------------------------------------------------
ACC_MAX_FUSED_CPW = 20480 // 32 - 12          # syrk_acc_max_fused_cpw
QUAD_MAX_CPG = 20480 // 8 - 12                # syrk_quad_max_cpg
OFF_LIMIT = 0xFFF00000


def num_blocks(K):
    return (K + 15) // 16


def quad_cluster(NB):
    return 1 if NB <= 18 else (2 if NB <= 23 else 4)


def short_phase_rows(K):
    return 112 if num_blocks(K) == 9 else 128


def waves_per_simd(K):
    NB = num_blocks(K)
    regs = 8 * (NB * (NB + 1) // 2) + 12 * NB + 40
    return max(1, min(8, 512 // regs))


def wave_p_max_fused_cpw(K, wg_per_cu):
    NB = num_blocks(K)
    fold = 2 * (NB * (NB + 1) // 2) * 256 * 8
    budget = max(min(160 * 1024 // max(wg_per_cu, 1), 64 * 1024), fold)
    return budget // 256 - 16


def pack_blocks(m):
    return max(1, min(512, (m + 2047) // 2048))


def plan(m, K, lda=None, *, nblocks=0, nsplit=0, short=-1, tiled=0, quad_min_rows=-1, fused_pack=1, num_cu=NUM_CU):
    """What fsnap_launch_info reports for these rows and options, with "family" added: 1P, 1A, 1S, 1Q, 1QC or 1T."""
    lda = K if lda is None else lda
    NB = num_blocks(K)
    nchunks = (m + 3) // 4
    info = {"compute_units": num_cu, "nsplit": 0}

    def quad_cpg():
        if tiled or K <= 144 or K > 512:
            return 0, 0
        cl = quad_cluster(NB)
        if cl > 1 and not fused_pack:
            return 0, 0
        min_rows = quad_min_rows if quad_min_rows >= 0 else (300000 if cl > 1 else 8192)
        if m < min_rows or m < 4:
            return 0, 0
        nb = (nblocks if nblocks > 0 else num_cu) // cl
        nb = max(1, min(nb, (nchunks + 23) // 24))
        cpg = (nchunks + nb - 1) // nb
        if cpg > OFF_LIMIT // (lda * 32) or (cl > 1 and cpg > QUAD_MAX_CPG):
            return 0, 0
        return cpg, (nchunks + cpg - 1) // cpg

    cpg, qblocks = quad_cpg()
    if tiled or (K > 144 and cpg == 0):
        if nsplit <= 0:
            raise NotImplementedError("the split model of tiled_geometry is not restated: force nsplit")
        NSB = (K + 63) // 64
        ns = max(1, min(nsplit, (nchunks + 31) // 32))
        cps = ((nchunks + ns - 1) // ns + 3) // 4 * 4
        ns = (nchunks + cps - 1) // cps
        npairs = NSB * (NSB + 1) // 2
        info.update(family="1T", workgroups=npairs * ns, threads=256, chunks_per_wave=cps // 4, NB=4 * NSB, split=0,
                    kernel_or_pairs=npairs, nsplit=ns)
        return info
    if NB >= 10:
        cl = quad_cluster(NB)
        info.update(family="1QC" if cl > 1 else "1Q", workgroups=qblocks, threads=256, chunks_per_wave=cpg, NB=NB, split=1,
                    kernel_or_pairs=6 if cl > 1 else 5, fused_pack=int(bool(fused_pack) and cpg <= QUAD_MAX_CPG))
        return info
    if NB >= 6 and short != 0 and (short == 1 or m <= 3 * short_phase_rows(K) * (num_cu // 2)):
        want = nblocks if nblocks > 0 else max(1, num_cu // 2)
        rpc = max(((m + want - 1) // want + 3) // 4 * 4, 32)
        info.update(family="1S", workgroups=(m + rpc - 1) // rpc, threads=512, chunks_per_wave=rpc, NB=NB, split=1,
                    kernel_or_pairs=7, fused_pack=int(bool(fused_pack)))
        return info
    if NB >= 6:
        nb = nblocks if nblocks > 0 else num_cu
        nb = max(1, min(nb, (nchunks + 47) // 48))
        cpw = min((nchunks + nb * 4 - 1) // (nb * 4), OFF_LIMIT // (lda * 32))
        nb = (nchunks + cpw * 4 - 1) // (cpw * 4)
        info.update(family="1A", workgroups=nb, threads=256, chunks_per_wave=cpw, NB=NB, split=1, kernel_or_pairs=3,
                    fused_pack=int(bool(fused_pack) and cpw <= ACC_MAX_FUSED_CPW))
        return info
    wg = waves_per_simd(K)
    nb = nblocks if nblocks > 0 else num_cu * wg
    nb = max(1, min(nb, (nchunks + 31) // 32))
    cpw = max(1, (nchunks + nb * 4 - 1) // (nb * 4))
    cpw = min(cpw, OFF_LIMIT // (lda * 32))
    nb = max(1, (nchunks + cpw * 4 - 1) // (cpw * 4))
    info.update(family="1P", workgroups=nb, threads=256, chunks_per_wave=cpw, NB=NB, split=1, kernel_or_pairs=4,
                fused_pack=int(bool(fused_pack) and cpw <= wave_p_max_fused_cpw(K, wg)))
    return info


def family_of(info):
    """Kernel family of a fsnap_launch_info dictionary."""
    if info["split"] == 0:
        return "1T"
    return {3: "1A", 4: "1P", 5: "1Q", 6: "1QC", 7: "1S"}[info["kernel_or_pairs"]]


# ---------------------------------------------------------------------------------------------------------------------------
# heights
# ---------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def red2_height(np_):
    return _cdiv(np_, 16) + 2 + 16


def red_tiled_height(np_, small_ok):
    return np_ if (small_ok and np_ <= 16) else _cdiv(np_, 16) + 2 + 16


def short_steps(rpc, RP):
    """4-row steps times four of a chunk of rpc rows staged in phases of RP rows, and the number of phases."""
    rows, phases, left = 0, 0, rpc
    while left > 0:
        nr = min(left, RP)
        rows += (nr + 7) & ~7
        phases += 1
        left -= nr
    return rows, phases


def depth(family, info, K, m=None, accumulate=False):
    """Additions a term passes through at most, {"G": h, "c": h, "s": h}, for the launch `info` (fsnap_launch_info) of `family`;
    the derivation per kernel, with file and line, is in the module docstring.  m (rows) sizes the packing kernel's partials
    when the pairs are not packed by the SYRK kernel itself; without it the launch's own upper bound is taken."""
    wg, cpw = info["workgroups"], info["chunks_per_wave"]
    NB = num_blocks(K)
    if family == "1T":
        ns = info["nsplit"]
        rows = m if m is not None else ns * cpw * 16
        npk = pack_blocks(rows)
        h = {"G": 4 * cpw + 2 + red_tiled_height(ns, True), "c": cpw + 2 + _cdiv(4 * ns, 16) + 16,
             "s": _cdiv(rows, npk * 256) + 8 + red_tiled_height(npk, False)}
    else:
        if family in ("1A", "1P"):
            rows_max = wg * cpw * 16
            g = 4 * cpw + (3 if family == "1A" else 2) + red2_height(wg)
            c = cpw + 2 + red2_height(4 * wg)
            sf = _cdiv(4 * cpw, 64) + 6 + red2_height(4 * wg)
        elif family == "1S":
            RP = short_phase_rows(K)
            RG = 512 // (8 * NB)
            steps, phases = short_steps(cpw, RP)
            rows_max = wg * cpw
            g = steps + red2_height(wg)
            c = _cdiv(RP, RG) * phases + (RG - 1) + red2_height(wg)
            sf = phases + 7 + red2_height(wg)
        elif family in ("1Q", "1QC"):
            cl = quad_cluster(NB)
            rows_max = wg * cpw * 4
            g = 4 * cpw + red2_height(wg)
            c = cpw + 2 + red2_height(4 * cl * wg)
            sf = _cdiv(4 * cpw, 256) + 6 + red2_height(4 * cl * wg)
        else:
            raise ValueError(family)
        if info.get("fused_pack", 1):
            s = sf
        else:
            rows = m if m is not None else rows_max
            npk = pack_blocks(rows)
            s = _cdiv(rows, npk * 256) + 8 + red2_height(npk)
        h = {"G": g, "c": c, "s": s}
    if accumulate:
        h = {k: v + 1 for k, v in h.items()}
    return h


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 mirror
# ---------------------------------------------------------------------------------------------------------------------------
class V:
    """A float64 array with the number of additions its terms have passed through at most."""
    __slots__ = ("a", "h")

    def __init__(self, a, h=0):
        self.a, self.h = a, h

    def __add__(self, o):
        return V(self.a + o.a, max(self.h, o.h) + 1)


def col_of(bq, e, NB, odd_last=True):
    if odd_last and (NB & 1) and bq == NB - 1:
        return 16 * bq + e
    return 32 * (bq >> 1) + 2 * e + (bq & 1)


def _perm(NB, K):
    """Column of A at place (block, element) of the kernels' interleave, -1 beyond K."""
    p = np.asarray([col_of(q, e, NB) for q in range(NB) for e in range(16)])
    return np.where(p < K, p, -1)


def _chain_ranges(family, info, m):
    """(partials, fold): partials = list of lists of (row0, row1) chains of the G accumulators; fold names how a partial's
    chains are combined."""
    wg, cpw = info["workgroups"], info["chunks_per_wave"]
    nchunks = (m + 3) // 4
    out = []
    if family in ("1A", "1P"):
        for g in range(wg):
            ch = []
            for rw in range(4):
                c0 = min((g * 4 + rw) * cpw, nchunks)
                c1 = min(c0 + cpw, nchunks)
                ch.append((4 * c0, min(4 * c1, m)))
            out.append(ch)
        return out, ("seq4" if family == "1A" else "tree4")
    if family == "1S":
        return [[(k * cpw, min((k + 1) * cpw, m))] for k in range(wg)], "one"
    if family in ("1Q", "1QC"):
        for g in range(wg):
            c0 = min(g * cpw, nchunks)
            c1 = min(c0 + cpw, nchunks)
            out.append([(4 * c0, min(4 * c1, m))])
        return out, "one"
    if family == "1T":
        cps = 4 * cpw
        for s in range(info["nsplit"]):
            s0 = s * cps
            s1 = min(s0 + cps, nchunks)
            ch = []
            for v in range(4):
                c0 = min(s0 + v * cpw, s1)
                c1 = min(c0 + cpw, s1)
                ch.append((4 * c0, min(4 * c1, m)))
            out.append(ch)
        return out, "tree4"
    raise ValueError(family)


def _reduce2(parts, faults=(), tiled=False):
    """Kernel 2b's order over a list of V partials (fsnap_reduce_partials2); tiled = fsnap_reduce_tiled's batches of 4 x 16."""
    n = len(parts)
    zero = V(np.zeros_like(parts[0].a), -10 ** 9)
    span, last = (64, 48) if tiled else (256, 240)
    red = []
    for s in range(16):
        a = [zero, zero, zero, zero]
        p = s
        while p + last < n:
            for j in range(span // 16):
                if 9 in faults and not tiled and 240 < n < 256 and j == 15:
                    continue
                a[j % 4] = a[j % 4] + parts[p + 16 * j]
            p += span
        while p < n:
            if not (8 in faults and n % 16 == 1 and p == n - 1):
                a[0] = a[0] + parts[p]
            p += 16
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    tot = red[0]
    for k in range(1, 16):
        tot = tot + red[k]
    if tot.h < 0:
        tot = V(tot.a, 0)
    return tot


def _seq(parts):
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    return tot


def _butterfly(v):
    """Sum of the 64 lanes by the xor butterfly (v: (64, ...) per wave); every lane ends with the same bits."""
    idx = np.arange(64)
    for sh in (1, 2, 4, 8, 16, 32):
        v = v + v[idx ^ sh]
    return v[0]


@dataclass
class Mirror:
    G: np.ndarray
    c: np.ndarray
    s: np.ndarray
    h: dict = field(default_factory=dict)


def mirror(case, family, info, K, faults=(), prev=None):
    """The statistics of `case` in float64 in the summation tree of `family` at the geometry `info`, with the switchable
    `faults`; prev = (G, c, s) makes it an accumulating launch.  Returns Mirror with the counted heights in .h."""
    faults = set(faults)
    A, b, w, t = case.A, case.b, case.w, case.testing
    m = A.shape[0]
    keep = ~t
    with np.errstate(invalid="ignore", over="ignore"):
        w_eff = w.copy() if 4 in faults else np.where(keep, w, 0.0)
        wbv = w_eff * b if 4 in faults else np.where(keep, w_eff * b, 0.0)
        live = w_eff != 0.0
        a = A.copy() if 5 in faults else np.where(live[:, None], A, 0.0)
        x = w_eff[:, None] * a
    if 1 in faults and m % 4:
        x = x.copy()
        x[m - m % 4:] = 0.0
        a = a.copy()
        a[m - m % 4:] = 0.0
    tiled = family == "1T"
    NB = info["NB"] if tiled else num_blocks(K)
    perm = _perm(NB, K)
    Kp = 16 * NB

    def gather(z):
        zp = np.zeros((m, Kp))
        ok = perm >= 0
        zp[:, ok] = z[:, perm[ok]]
        return zp

    with np.errstate(invalid="ignore", over="ignore"):
        xp = gather(x)
        if 12 in faults:
            xp[:, :16] = xp[:, :16].astype(np.float32).astype(np.float64)
        if tiled:
            yp = gather((w_eff * w_eff)[:, None] * a)          # (w^2 a_I) on the left of an off-diagonal superblock pair ...
            ap = gather(a)                                      # ... a_J as loaded on the right
            if 12 in faults:
                yp[:, :16] = yp[:, :16].astype(np.float32).astype(np.float64)
            sb = np.arange(Kp) // 64
            same_sb = sb[:, None] == sb[None, :]

        # ---- G: chains -> fold -> partials -> reduction --------------------------------------------------------------------
        partials, fold = _chain_ranges(family, info, m)

        def chain(r0, r1):
            if 2 in faults and r1 < m and r1 > r0:
                r1 = min(r1 + 4, m)
            if 3 in faults and family in ("1A", "1Q", "1QC") and r1 > r0:
                ncl = (r1 - r0 + 3) // 4
                cl = 0
                while cl + 3 < ncl:
                    cl += 6
                if cl < ncl:                      # the half trip runs: its last chunk is lost
                    r1 = r0 + 4 * (ncl - 1)
            acc = np.zeros((Kp, Kp))
            for r in range(r0, r1):
                acc = acc + np.outer(xp[r], xp[r])
            if tiled:
                off = np.zeros((Kp, Kp))
                for r in range(r0, r1):
                    off = off + np.outer(yp[r], ap[r])
                acc = np.where(same_sb, acc, off)
            return V(acc, r1 - r0 if r1 > r0 else -10 ** 9)

        gparts = []
        for ip, chs in enumerate(partials):
            vs = [chain(*rr) for rr in chs]
            if fold == "seq4":
                p = ((vs[0] + vs[1]) + vs[2]) + vs[3]
            elif fold == "tree4":
                p = (vs[0] + vs[2]) + (vs[1] + vs[3])
            else:
                p = vs[0]
            if 13 in faults and ip == len(partials) // 2:
                p = V(p.a.astype(np.float32).astype(np.float64), p.h)
            gparts.append(V(p.a, max(p.h, 0)))
        if tiled and len(gparts) <= 16:
            gt = _seq([V(np.zeros((Kp, Kp)), -10 ** 9)] + gparts)       # fsnap_reduce_tiled_small: tot = 0 + p0 + p1 ...
        else:
            gt = _reduce2(gparts, faults, tiled=tiled)
        # scatter: undo the interleave, mirror the triangle (tiles p <= q only)
        G = np.zeros((K, K)) if prev is None else prev[0].copy()
        rowc = np.asarray([col_of(q, e, NB, odd_last=6 not in faults) for q in range(NB) for e in range(16)])
        rowc = rowc if not tiled else perm.copy()
        for p in range(NB):
            for q in range(p, NB):
                tile = gt.a[16 * p:16 * p + 16, 16 * q:16 * q + 16]
                r, c = rowc[16 * p:16 * p + 16], rowc[16 * q:16 * q + 16]
                ok = (r[:, None] < K) & (c[None, :] < K) & (r[:, None] >= 0) & (c[None, :] >= 0)
                rr, cc = np.broadcast_to(r[:, None], (16, 16))[ok], np.broadcast_to(c[None, :], (16, 16))[ok]
                val = tile[ok] + (G[rr, cc] if prev is not None else 0.0)
                G[rr, cc] = val
                if p != q:
                    if 7 in faults:          # the tile copied, not transposed, into block (q, p)
                        ok2 = (c[:, None] < K) & (c[:, None] >= 0) & (r[None, :] < K) & (r[None, :] >= 0)
                        G[np.broadcast_to(c[:, None], (16, 16))[ok2], np.broadcast_to(r[None, :], (16, 16))[ok2]] = tile[ok2]
                    else:
                        G[cc, rr] = val
        hG = gt.h + (1 if prev is not None else 0)

        # ---- c -------------------------------------------------------------------------------------------------------------
        wbc = wbv.copy()
        if 10 in faults:
            idx = np.arange(m) ^ 1
            wbc = np.where(idx < m, wbv[np.minimum(idx, m - 1)], 0.0)
        xc = xp                                                 # (c rides on the operands of the diagonal tiles)
        cparts = []

        def lanes_chain(r0, r1, step, nlane):
            """nlane interleaved chains over rows r0 + lane, r0 + lane + step, ...: (nlane, Kp) sums and the chain length."""
            acc = np.zeros((nlane, Kp))
            n = 0
            for base in range(r0, r1, step):
                rows = np.arange(base, min(base + nlane, r1))
                acc[:rows.size] = acc[:rows.size] + xc[rows] * wbc[rows][:, None]
                n += 1
            return acc, n

        if family == "1S":
            RP, RG = short_phase_rows(K), 512 // (8 * num_blocks(K))
            for ((r0, r1),) in partials:
                acc = np.zeros((RG, Kp))
                n = 0
                for ph0 in range(r0, r1, RP):             # thread (rg, u): rows rg, rg + RG, ... of every phase
                    ph1 = min(ph0 + RP, r1)
                    for base in range(ph0, ph1, RG):
                        rows = np.arange(base, min(base + RG, ph1))
                        acc[:rows.size] = acc[:rows.size] + xc[rows] * wbc[rows][:, None]
                        n += 1
                cparts.append(_seq([V(acc[k], n) for k in range(RG)]))
        else:
            for chs in partials:
                for (r0, r1) in chs:
                    acc, n = lanes_chain(r0, r1, 4, 4)
                    k = [V(acc[i], n) for i in range(4)]
                    cparts.append((k[0] + k[1]) + (k[2] + k[3]))
                if family in ("1Q", "1QC"):
                    for _ in range(4 * quad_cluster(num_blocks(K)) - 1):   # the waves that do not own the block store zeros
                        cparts.append(V(np.zeros(Kp), 0))
        if tiled:
            red = []
            zero = V(np.zeros(Kp), -10 ** 9)
            for g in range(16):
                sacc = zero
                for q in range(g, len(cparts), 16):
                    sacc = sacc + cparts[q]
                red.append(sacc)
            ct = _seq([zero] + red)
        else:
            ct = _reduce2(cparts, faults)
        base_c = np.zeros(K) if (prev is None or 11 in faults) else prev[1]
        c = base_c.copy()
        okc = (rowc >= 0) & (rowc < K)
        c[rowc[okc]] = base_c[rowc[okc]] + ct.a[okc]
        hc = max(ct.h, 0) + (1 if prev is not None else 0)

        # ---- scalars ---------------------------------------------------------------------------------------------------------
        cnt = np.where(keep, 1.0, 0.0)
        trip = np.stack([wbv * wbv, wbv, cnt], axis=1)                  # (m, 3)

        def strided(r0, r1, nthr):
            acc = np.zeros((nthr, 3))
            n = 0
            for base in range(r0, r1, nthr):
                rows = np.arange(base, min(base + nthr, r1))
                acc[:rows.size] = acc[:rows.size] + trip[rows]
                n += 1
            return acc, n

        sparts = []
        if tiled or not info.get("fused_pack", 1):
            npk = pack_blocks(m)
            for blk_ in range(npk):
                acc = np.zeros((256, 3))
                n = 0
                for base in range(blk_ * 256, m, npk * 256):
                    rows = np.arange(base, min(base + 256, m))
                    acc[:rows.size] = acc[:rows.size] + trip[rows]
                    n += 1
                sft = 128
                while sft > 0:
                    acc[:sft] = acc[:sft] + acc[sft:2 * sft]
                    sft >>= 1
                sparts.append(V(acc[0].copy(), n + 8))
        elif family in ("1A", "1P"):
            for chs in partials:
                for (r0, r1) in chs:
                    acc, n = strided(r0, r1, 64)
                    sparts.append(V(_butterfly(acc), n + 6))
        elif family in ("1Q", "1QC"):
            for ((r0, r1),) in partials:
                acc, n = strided(r0, r1, 256)
                for wv in range(4):
                    sparts.append(V(_butterfly(acc[64 * wv:64 * wv + 64]), n + 6))
                for _ in range(4 * (quad_cluster(num_blocks(K)) - 1)):
                    sparts.append(V(np.zeros(3), 0))
        elif family == "1S":
            RP = short_phase_rows(K)
            for ((r0, r1),) in partials:
                acc = np.zeros((128, 3))
                n = 0
                for ph0 in range(r0, r1, RP):
                    rows = np.arange(ph0, min(ph0 + RP, r1))
                    acc[:rows.size] = acc[:rows.size] + trip[rows]
                    n += 1
                sparts.append(V(_butterfly(acc[:64]) + _butterfly(acc[64:]), n + 7))
        if tiled:
            st = _reduce2(sparts, faults, tiled=True)
        else:
            st = _reduce2(sparts, faults)
        s = st.a[:3] if prev is None else prev[2] + st.a[:3]
        hs = max(st.h, 0) + (1 if prev is not None else 0)
    return Mirror(G, c, np.asarray(s, dtype=np.float64), {"G": hG, "c": hc, "s": hs})


# ---------------------------------------------------------------------------------------------------------------------------
# the sweeps: (kernel, K, rows, options) -- shared by the CPU run (mirror) and the GPU run (kernels)
# ---------------------------------------------------------------------------------------------------------------------------
OPTION_DEFAULTS = {"nblocks": 0, "nsplit": 0, "short": -1, "tiled": 0, "quad_min_rows": -1, "fused_pack": 1}


@dataclass(frozen=True)
class Geo:
    kernel: str                    # the family that must run
    K: int
    m: int
    opts: tuple = ()               # ((option, value), ...) away from OPTION_DEFAULTS
    lda: int = 0                   # 0 = K; otherwise the rows are bound in place with this leading dimension
    want: tuple = ()               # ((launch_info key, value), ...) the sweep intends beyond the kernel

    def options(self):
        return dict(self.opts)

    def info(self):
        info = plan(self.m, self.K, self.lda or None, **self.options())
        assert info["family"] == self.kernel, (self, info)
        for k, v in self.want:
            assert info[k] == v, (self, k, info)
        return info


def _geo(kernel, K, m, want=(), lda=0, **opts):
    return Geo(kernel, K, m, tuple(sorted(opts.items())), lda, tuple(want))


K_1A = (81, 96, 97, 112, 113, 128, 129, 142, 144)
K_1P = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80)
K_1S = (81, 96, 110, 128, 129, 142, 144)
K_1Q = (145, 150, 168, 180, 200, 220, 230, 250, 264, 275, 288)         # NB = 10 ... 18, once each, and the two ends
K_1QC = (289, 304, 368, 369, 384, 480, 512)
K_1T = (31, 64, 128, 145, 192, 193, 256, 257, 320, 512, 513, 1000, 1595)
NP_REDUCE = (1, 2, 15, 16, 17, 31, 32, 33, 239, 240, 241, 255, 256, 257, 271, 272, 273, 511, 512, 513)
K_REDUCE = {"1P": (16, 33), "1A": (96, 142)}


def sweep_1a(K):
    out = []
    for fused in (1, 0):
        for n in range(1, 15):                       # chunks per wave 1 ... 14 in one workgroup: ragged last chunk (r = 1, 3),
            for r in (0, 1, 3, 4, 8, 12):            # a shorter last wave (4, 8) and an empty one (12)
                if 16 * n - r >= 1:
                    out.append(_geo("1A", K, 16 * n - r, [("chunks_per_wave", n), ("workgroups", 1), ("fused_pack", fused)],
                                    short=0, nblocks=1, fused_pack=fused))
    for nb in (2, 3, 17):
        for i, n in enumerate(range(12, 19)):        # 12 ... 18: the chunks per wave modulo 6, full and half trips
            r = (0, 3, 5)[(i + nb) % 3]
            out.append(_geo("1A", K, 16 * nb * n - r, [("chunks_per_wave", n), ("workgroups", nb)], short=0, nblocks=nb))
            if nb == 3:
                out.append(_geo("1A", K, 16 * nb * n - r, [("chunks_per_wave", n), ("workgroups", nb), ("fused_pack", 0)],
                                short=0, nblocks=nb, fused_pack=0))
    n = ACC_MAX_FUSED_CPW + 1                        # the pairs no longer fit the LDS: pairs from HBM although fused_pack = 1
    out.append(_geo("1A", K, 16 * n - 3, [("chunks_per_wave", n), ("workgroups", 1), ("fused_pack", 0)], short=0, nblocks=1))
    return out


def sweep_1p(K):
    out = []
    for fused in (1, 0):
        for n in list(range(1, 21)) + [31, 32, 33]:
            for r in (0, 1, 5):
                out.append(_geo("1P", K, 16 * n - r, [("chunks_per_wave", n), ("workgroups", 1), ("fused_pack", fused)],
                                nblocks=1, fused_pack=fused))
        for n in (31, 32, 33):
            out.append(_geo("1P", K, 32 * n - 3, [("chunks_per_wave", n), ("workgroups", 2), ("fused_pack", fused)],
                            nblocks=2, fused_pack=fused))
    if K & 1:                                        # rows only 8-byte aligned: bound in place with an odd leading dimension
        for n in (1, 7, 18, 32):
            out.append(_geo("1P", K, 16 * n - 1, [("chunks_per_wave", n)], lda=K + 8, nblocks=1))
    return out


def sweep_1s(K):
    RP = short_phase_rows(K)
    out = []
    lengths = (32, RP - 4, RP + 4, 2 * RP - 4, 2 * RP + 4, 3 * RP - 4, 3 * RP + 4)
    for i, rpc in enumerate(lengths):
        for j, nb in enumerate((1, 3, 7, 8, 9, 17)):
            r = (0, 1, 3)[(i + j) % 3]
            out.append(_geo("1S", K, nb * rpc - r, [("chunks_per_wave", rpc), ("workgroups", nb), ("fused_pack", 1)], nblocks=nb))
        out.append(_geo("1S", K, 3 * rpc - 2, [("chunks_per_wave", rpc), ("workgroups", 3), ("fused_pack", 0)], nblocks=3,
                        fused_pack=0))                # pairs from HBM
    return out


def sweep_1q(K):
    out = []
    for n in list(range(1, 15)) + [23, 24, 25]:      # six-chunk trips and the half trip, one workgroup
        for r in (0, 1, 3):
            if 4 * n - r >= 4:                       # (fewer than four rows stay on the tiled kernel)
                out.append(_geo("1Q", K, 4 * n - r, [("chunks_per_wave", n), ("workgroups", 1), ("fused_pack", 1)],
                                quad_min_rows=0, nblocks=1))
        out.append(_geo("1Q", K, max(4 * n - 2, 4), [("chunks_per_wave", n), ("workgroups", 1), ("fused_pack", 0)], quad_min_rows=0,
                        nblocks=1, fused_pack=0))
    for nb in (2, 5):
        for i, n in enumerate((24, 25, 30)):
            out.append(_geo("1Q", K, 4 * nb * n - (0, 1, 3)[i], [("chunks_per_wave", n), ("workgroups", nb)], quad_min_rows=0,
                            nblocks=nb))
    return out


def sweep_1qc(K):
    cl = quad_cluster(num_blocks(K))
    out = []
    for n in list(range(1, 9)) + [24, 25, 26]:
        for r in (0, 3):
            if 4 * n - r >= 4:
                out.append(_geo("1QC", K, 4 * n - r, [("chunks_per_wave", n), ("workgroups", 1)], quad_min_rows=0, nblocks=cl))
    for ncl in (2, 3):                               # (the planner gives a cluster at least 24 chunks before it adds one)
        for i, n in enumerate((24, 25, 26)):
            out.append(_geo("1QC", K, 4 * ncl * n - (0, 1, 3)[i], [("chunks_per_wave", n), ("workgroups", ncl)], quad_min_rows=0,
                            nblocks=ncl * cl))
    return out


def sweep_1t(K):
    out = []
    for n in (1, 2, 3):                              # one split of 1 ... 3 chunks: waves with one chunk and with none
        for r in (0, 1, 3):
            out.append(_geo("1T", K, 4 * n - r, [("nsplit", 1), ("chunks_per_wave", 1)], tiled=1, nsplit=1))
    for s in (1, 2, 7, 16, 17, 33):
        # tiled_geometry keeps >= 32 chunks per split (8 per wave) from the second split on: 8, 9 and 10 chunks per wave are the
        # shortest splits the options reach -- the 1 ... 3 chunks per split of more than one split are not reachable
        # (the long-double reference of 4 000 ... 5 000 rows costs seconds from K = 192 on: every pair of rows and remainder up to
        # K = 145, one remainder per length beyond, one length from 16 splits on at K >= 512)
        for i, cpw in enumerate((8, 9, 10) if (K <= 320 or s <= 7) else (8,)):
            for r in ((0, 1, 3) if K <= 145 else ((0, 1, 3)[(i + 1) % 3 if K > 320 and s > 7 else i],)):
                out.append(_geo("1T", K, 16 * s * cpw - r, [("nsplit", s), ("chunks_per_wave", cpw)], tiled=1, nsplit=s))
    return out


def reduce_rows(kernel, nb):
    """Fewest rows at which the planner keeps nb workgroups (kernel 1P: 32 chunks per workgroup, kernel 1A: 48)."""
    per = 32 if kernel == "1P" else 48
    return 4 * (per * (nb - 1) + 1)


def sweep_reduce(kernel, K):
    """(geometry of the batch under test, rows of the second batch of an accumulating pair)."""
    out = []
    for nb in NP_REDUCE:
        if kernel == "1A" and nb > 257:
            continue
        opts = {"nblocks": nb}
        if kernel == "1A":
            opts["short"] = 0
        out.append((_geo(kernel, K, reduce_rows(kernel, nb), [("workgroups", nb)], **opts), 331))
    return out


SWEEPS = {"1A": (sweep_1a, K_1A), "1P": (sweep_1p, K_1P), "1S": (sweep_1s, K_1S), "1Q": (sweep_1q, K_1Q),
          "1QC": (sweep_1qc, K_1QC), "1T": (sweep_1t, K_1T)}


def second_batch_opts(kernel):
    """Options of the small second batch of an accumulating pair: the planner's own choice (kernel 1A kept off kernel 1S)."""
    return {"short": 0} if kernel == "1A" else {}


def half_trip(n_chunks):
    """Does kernel 1A's / 1Q's loop end with the half trip for a wave of n_chunks chunks?"""
    cl = 0
    while cl + 3 < n_chunks:
        cl += 6
    return cl < n_chunks


def can_act(fault, geo, info, case=None, accumulate=False):
    """Can `fault` change the statistics of this launch at all?"""
    partials, _ = _chain_ranges(geo.kernel, info, geo.m)
    chains = [rr for chs in partials for rr in chs if rr[1] > rr[0]]
    nps = {"1T": ()}.get(geo.kernel)
    if nps is None:
        wg = info["workgroups"]
        cs = {"1S": 1, "1Q": 4, "1QC": 4 * quad_cluster(num_blocks(geo.K))}.get(geo.kernel, 4)
        nps = (wg, wg * cs, wg * cs if info.get("fused_pack", 1) else pack_blocks(geo.m))
    else:
        nps = ((info["nsplit"],) if info["nsplit"] > 16 else ()) + (pack_blocks(geo.m),)
    if fault == 1:
        return geo.m % 4 != 0
    if fault == 2:
        return any(r1 < geo.m for _, r1 in chains)
    if fault == 3:
        return geo.kernel in ("1A", "1Q", "1QC") and any(half_trip((r1 - r0 + 3) // 4) for r0, r1 in chains)
    if fault == 4:
        return case is None or bool(case.testing.any())
    if fault == 5:
        return case is None or bool(((case.w == 0.0) & ~case.testing).any())
    if fault == 6:
        # (a last block of one column is column 16 (NB - 1) in either order)
        return geo.kernel != "1T" and num_blocks(geo.K) % 2 == 1 and geo.K - 16 * (num_blocks(geo.K) - 1) >= 2
    if fault == 7:
        return geo.K > 16
    if fault == 8:
        # (slice 0 takes partial np - 1 in its tail unless a batch ends exactly there: np = 241 mod 256, 49 mod 64 when tiled)
        span, last = (64, 48) if geo.kernel == "1T" else (256, 240)
        return any(n % 16 == 1 and n % span != last + 1 for n in nps)
    if fault == 9:
        return geo.kernel != "1T" and any(240 < n < 256 for n in nps)
    if fault == 10:
        return geo.m >= 2
    if fault == 11:
        return accumulate
    return True
