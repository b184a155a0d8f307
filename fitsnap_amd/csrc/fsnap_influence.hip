// fsnap_influence.hip — per-configuration influence vectors and the outer-product sums of the cluster-robust coefficient
// covariances of a linear smoother (gfx950 only).
//
// With the conventions of fsnap_loco.hip (zeta_i = a_i M, z_i = w_i zeta_i, e_i = w_i b_i - w_i (a_i . beta)), per unit c:
//     s_c = Z_c^T e_c                       the score of the unit in M space (no solve)
//     v_c = (I - Z_c^T Z_c)^-1 s_c          kernel L2's v: beta_{-c} = beta - M v_c
//     W_s = sum_c s_c s_c^T,  W_v = sum_{c identifiable} v_c v_c^T
//
//   I1  fsnap_infl_cfg_k<D>     kernel L2 / L3's geometry (one workgroup of 4 waves per unit, grid-stride over a bin's list;
//                               D = 32 / 64 / 128 in LDS, D = 0 on a slice of global scratch).  Per unit loco_one_cfg<true>
//                               (fsnap_loco_body.h) unchanged, so the predictions and the four info columns are those of
//                               fsnap_loco_cfg_k bit for bit; afterwards v is still in the body's buffers (vbuf in n space, r in
//                               J space) and, in J space, s_c in r0.  In n space the epilogue forms s_c[a] by the body's own
//                               loop over the unit's rows.  Writes V[c] (zeros when not identifiable), S[c] and
//                               unit[c] = (|v_c|^2, |s_c|^2, s_c . v_c) (first and third NaN when not identifiable).
//   I0  fsnap_infl_scores_k     s_c alone: one workgroup per unit, thread a sums fma(w_i zeta_i[a], e_i, .) over the unit's
//                               positions in order -- the statement of the body's J-space right-hand side and of I1's n-space
//                               epilogue, so S[c] and |s_c|^2 are BIT-IDENTICAL to I1's in either space.  unit[c] =
//                               (NaN, |s_c|^2, NaN): no v.
//   I2  fsnap_infl_outer_k      W = X^T X of X (nunits x Jp, row-major) on v_mfma_f64_16x16x4f64: one wave per (lower 16 x 16
//       fsnap_infl_fold_k       tile, chunk of 512 units) accumulates the chunk's units in index order, 4 per MFMA step (units
//                               past the end contribute zeros), and stores its tile to part[chunk][tile]; the fold adds the
//                               chunks in index order and mirrors the triangle.  Bit-identical run to run; the sums depend on
//                               the ORDER of the units (the chunking and the accumulation order), so W is not invariant under
//                               a permutation of the units.
// The norms are summed in a fixed order over a: thread t adds a = t, t + 256, ... in order, then the wave butterfly of
// fsnap_wave_sum.h, then waves 0 ... 3 in order.  A unit's V, S and unit record depend on its own rows alone: bit-identical
// run to run and under any permutation or subset of the units.  fp64 only, no atomics; plain vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_loco_body.h"
#include "fsnap_wave_sum.h"

namespace {

constexpr int INFL_CHUNK = fsnap::INFL_CHUNK;

// s_c[a] = sum_i (w_i zeta_i[a]) e_i over the unit's positions in order: the body's J-space right-hand side, statement for
// statement
__device__ __forceinline__ double infl_score(const double* __restrict__ Zc, int Jp, const double* __restrict__ pw,
                                             const double* __restrict__ pe, int64_t base, int n, int a) {
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) s = __builtin_fma(pw[base + i] * Zc[(int64_t)i * Jp + a], pe[base + i], s);
    return s;
}

// The three per-thread partials (over a = tid, tid + 256, ...) -> wave butterfly -> waves 0 ... 3 in order; thread 0 writes
// the record.  red: 12 doubles of LDS.  Ends with a barrier (red is reused by the next unit).
__device__ __forceinline__ void infl_unit_record(double vv, double ss, double sv, bool have_v, double* red,
                                                 double* __restrict__ unit_c) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    vv = wave_sum(vv);
    ss = wave_sum(ss);
    sv = wave_sum(sv);
    if (lane == 0) {
        red[3 * wave] = vv;
        red[3 * wave + 1] = ss;
        red[3 * wave + 2] = sv;
    }
    __syncthreads();
    if (tid == 0) {
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = ((red[k] + red[3 + k]) + red[6 + k]) + red[9 + k];
        const double nan = __builtin_nan("");
        unit_c[0] = have_v ? t[0] : nan;
        unit_c[1] = t[1];
        unit_c[2] = have_v ? t[2] : nan;
    }
    __syncthreads();
}

// H, r, r0, gd as loco_one_cfg<true> takes them; red: 12 doubles of LDS.
__device__ __forceinline__ void infl_one_cfg(const double* __restrict__ Z, int Jp, int J, const double* __restrict__ pw,
                                             const double* __restrict__ pe, const double* __restrict__ pb,
                                             const int* __restrict__ idx, int64_t base, int n, double* H, int ldh, double* r,
                                             double* r0, double* gd, double* red, double* __restrict__ vbuf,
                                             double* __restrict__ pred, double* __restrict__ info_c, double* __restrict__ V_c,
                                             double* __restrict__ S_c, double* __restrict__ unit_c) {
    const int tid = threadIdx.x;
    const bool nspace = n <= J;
    const bool ok = loco_one_cfg<true>(Z, Jp, J, pw, pe, pb, idx, base, n, H, ldh, r, vbuf, pred, info_c, gd, r0);
    // the body ended on a barrier: r / vbuf (v) and r0 (s_c, J space) are complete
    const double* Zc = Z + base * Jp;
    const double* v = nspace ? vbuf : r;
    double vv = 0.0, ss = 0.0, sv = 0.0;
    for (int a = tid; a < Jp; a += 256) {
        double s = 0.0, va = 0.0;
        if (a < J) {
            s = nspace ? infl_score(Zc, Jp, pw, pe, base, n, a) : r0[a];
            if (ok) va = v[a];
        }
        S_c[a] = s;
        V_c[a] = va;
        vv = __builtin_fma(va, va, vv);
        ss = __builtin_fma(s, s, ss);
        sv = __builtin_fma(s, va, sv);
    }
    infl_unit_record(vv, ss, sv, ok, red, unit_c);    // its barriers also fence r, r0, vbuf against the next unit
}

template <int D>
__global__ __launch_bounds__(256) void fsnap_infl_cfg_k(const double* __restrict__ Z, int Jp, int J,
                                                        const double* __restrict__ pw, const double* __restrict__ pe,
                                                        const double* __restrict__ pb, const int* __restrict__ idx,
                                                        const int64_t* __restrict__ off, const int* __restrict__ clist,
                                                        int ncl, double* __restrict__ Hg, int dmax, double* __restrict__ vg,
                                                        double* __restrict__ pred, double* __restrict__ info,
                                                        double* __restrict__ V, double* __restrict__ S,
                                                        double* __restrict__ unit) {
    double* vbuf = vg + (int64_t)blockIdx.x * Jp;
    __shared__ double sred[12];
    if constexpr (D > 0) {
        __shared__ double sH[D * D];
        __shared__ double sr[3 * D];
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            infl_one_cfg(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), sH, D, sr, sr + D, sr + 2 * D, sred,
                         vbuf, pred, info + 4 * (int64_t)c, V + (int64_t)c * Jp, S + (int64_t)c * Jp, unit + 3 * (int64_t)c);
        }
    } else {
        double* H = Hg + (int64_t)blockIdx.x * fsnap::loco_uq_scratch_doubles(dmax);
        double* r = H + (int64_t)dmax * dmax;
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            infl_one_cfg(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), H, dmax, r, r + dmax, r + 2 * dmax,
                         sred, vbuf, pred, info + 4 * (int64_t)c, V + (int64_t)c * Jp, S + (int64_t)c * Jp,
                         unit + 3 * (int64_t)c);
        }
    }
}

__global__ __launch_bounds__(256) void fsnap_infl_scores_k(const double* __restrict__ Z, int Jp, int J,
                                                           const double* __restrict__ pw, const double* __restrict__ pe,
                                                           const int64_t* __restrict__ off, const int* __restrict__ clist,
                                                           int ncl, double* __restrict__ S, double* __restrict__ unit) {
    __shared__ double sred[12];
    const int tid = threadIdx.x;
    for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
        const int c = clist[q];
        const int64_t base = off[c];
        const int n = (int)(off[c + 1] - base);
        const double* Zc = Z + base * Jp;
        double* S_c = S + (int64_t)c * Jp;
        double ss = 0.0;
        for (int a = tid; a < Jp; a += 256) {
            const double s = a < J ? infl_score(Zc, Jp, pw, pe, base, n, a) : 0.0;
            S_c[a] = s;
            ss = __builtin_fma(s, s, ss);
        }
        infl_unit_record(0.0, ss, 0.0, false, sred, unit + 3 * (int64_t)c);
    }
}

// one wave per (tile, chunk): blockIdx.x = chunk * ntiles + tile
__global__ __launch_bounds__(64) void fsnap_infl_outer_k(const double* __restrict__ X, int64_t nunits, int Jp, int ntiles,
                                                         double* __restrict__ part) {
    const int lane = threadIdx.x, e = lane & 15, ks = lane >> 4;
    const int t = (int)(blockIdx.x % (unsigned)ntiles);
    const int64_t chunk = blockIdx.x / (unsigned)ntiles;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    // A operand lane (e, ks): X[u0 + 4 s + ks][16 ti + e]; B operand: X[u0 + 4 s + ks][16 tj + e]   (fsnap_loco_body.h, J space)
    const int ca = 16 * ti + e, cb = 16 * tj + e;
    const int64_t u0 = chunk * INFL_CHUNK;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < INFL_CHUNK / 4; ++s) {
        const int64_t u = u0 + 4 * s + ks;
        double xa = 0.0, xb = 0.0;
        if (u < nunits) {
            xa = X[u * Jp + ca];
            xb = X[u * Jp + cb];
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
    }
    // D[reg g] at lane (e, ks) = W[16 ti + ks + 4 g][16 tj + e]
    double* dst = part + ((int64_t)blockIdx.x << 8);
#pragma unroll
    for (int g = 0; g < 4; ++g) dst[16 * (ks + 4 * g) + e] = acc[g];
}

// W (J x J): tile t of every chunk added in chunk order; the strict upper triangle is the mirror of the lower one (a diagonal
// tile holds both halves, bitwise equal: the same products in the same order)
__global__ __launch_bounds__(256) void fsnap_infl_fold_k(const double* __restrict__ part, int64_t nchunks, int ntiles, int J,
                                                         double* __restrict__ W) {
    const int t = blockIdx.x;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int i = 16 * ti + ((int)threadIdx.x >> 4), j = 16 * tj + ((int)threadIdx.x & 15);
    double s = 0.0;
    for (int64_t ch = 0; ch < nchunks; ++ch) s += part[((ch * ntiles + t) << 8) + threadIdx.x];
    if (i < J && j < J) {
        W[(int64_t)i * J + j] = s;
        if (ti != tj) W[(int64_t)j * J + i] = s;
    }
}

}  // namespace

namespace fsnap {

hipError_t launch_infl_cfg(int D, int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                           const double* pb, const int* idx, const int64_t* off, const int* clist, int ncl, double* Hg,
                           int dmax, double* vg, double* pred, double* info, double* V, double* S, double* unit,
                           hipStream_t st) {
    if (ncl <= 0 || nblocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)nblocks);
    const bool known = dispatch_d(D, [&](auto dd) {
        fsnap_infl_cfg_k<decltype(dd)::value><<<grid, 256, 0, st>>>(Z, Jp, J, pw, pe, pb, idx, off, clist, ncl, Hg, dmax, vg, pred, info, V, S, unit);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_infl_scores(int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                              const int64_t* off, const int* clist, int ncl, double* S, double* unit, hipStream_t st) {
    if (ncl <= 0 || nblocks <= 0) return hipSuccess;
    fsnap_infl_scores_k<<<dim3((unsigned)nblocks), 256, 0, st>>>(Z, Jp, J, pw, pe, off, clist, ncl, S, unit);
    return hipGetLastError();
}

hipError_t launch_infl_outer(const double* X, int64_t nunits, int Jp, int J, double* part, double* W, hipStream_t st) {
    if (nunits <= 0) return hipSuccess;
    const int nt = Jp / 16, ntiles = nt * (nt + 1) / 2;
    const int64_t nchunks = infl_chunks(nunits);
    if (nchunks * ntiles > 0x7FFFFFFF) return hipErrorInvalidValue;
    fsnap_infl_outer_k<<<dim3((unsigned)(nchunks * ntiles)), 64, 0, st>>>(X, nunits, Jp, ntiles, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    fsnap_infl_fold_k<<<dim3((unsigned)ntiles), 256, 0, st>>>(part, nchunks, ntiles, J, W);
    return hipGetLastError();
}

}  // namespace fsnap
