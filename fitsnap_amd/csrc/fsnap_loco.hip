// fsnap_loco.hip — exact leave-one-configuration-out (LOCO) predictions of a linear smoother (gfx950 only).
//
// Given the training rows a_i (resident), their packed weights (w_i, w_i b_i) (kernel 1A's wpack: w_i = 0 off the mask),
// a factor M (K x J) of C = (G + alpha I)^-1 = M M^T and the fit beta, for every configuration c (a run of positions
// [off[c], off[c + 1]) of a configuration-sorted row index idx):
//     zeta_i = a_i M,  z_i = w_i zeta_i,  e_i = w_i b_i - w_i (a_i . beta)
//     n space (n_c <= J):  u = (I - Z_c Z_c^T)^-1 e_c,  v = Z_c^T u
//     J space (n_c >  J):  v = (I - Z_c^T Z_c)^-1 Z_c^T e_c
//     LOO prediction of every row i of c:  p_i = a_i . beta - zeta_i . v        (= a_i . beta_{-c}, Woodbury)
//
//   L1  fsnap_loco_zeta_k<NT>   one pass over the index positions: zeta (npos x Jp, by position) on
//                               v_mfma_f64_16x16x4f64 with the M tile as the A operand and the row block as the B operand
//                               (fsnap_uq.hip U1's lane mapping: D[reg g] at lane (e, ks) is zeta_e[16 jt + ks + 4 g]),
//                               plus a_i . beta, w_i and e_i per position.  NT = ceil(K / 16) <= 9 keeps the rows in
//                               registers; NT = 0 (K > 144, untuned) re-reads them (L1 / L2) per M tile.
//   L2  fsnap_loco_cfg_k<D>     one workgroup (4 waves) per configuration, grid-stride over a list of configurations
//                               whose d_c = min(n_c, J) <= D: the d_c x d_c matrix H = I - (Gram) is built in LDS on MFMA
//                               (16 x 16 lower tiles, one wave per tile), factorised by a right-looking Cholesky in LDS
//                               with a pivot check, solved, and p_i written for every row of c.  D = 0: the same code on
//                               a slice of global scratch per workgroup (d_c > 128, untuned).  Its per-configuration body,
//                               loco_one_cfg, is in fsnap_loco_body.h: kernel L3 of fsnap_loco_uq.hip runs it too.
// A configuration whose smallest pivot is <= LOCO_PIVOT_TOL (lambda_max(S_c) -> 1: not identifiable without itself) is
// never divided through: its rows get NaN and its info record says so.  Every sum runs in a fixed order that depends on the
// configuration's own rows only (zeta_i on a_i and M alone, as in fsnap_uq.hip), so a row's result is bit-identical under
// repeats and under any permutation of the configurations.  No atomics; results are written with vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_loco_body.h"
#include "fsnap_wave_sum.h"

namespace {

constexpr int LOCO_RB = 2;   // 16-position blocks per wave in kernel L1

template <int NT>
__global__ __launch_bounds__(256) void fsnap_loco_zeta_k(const double* __restrict__ A, int64_t lda, int K,
                                                         const int* __restrict__ idx, int64_t npos,
                                                         const double* __restrict__ wpack, const double* __restrict__ Mp,
                                                         int Jp, const double* __restrict__ bp, double* __restrict__ Z,
                                                         double* __restrict__ pw, double* __restrict__ pe,
                                                         double* __restrict__ pb) {
    constexpr int NS = NT > 0 ? 4 * NT : 1;
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * LOCO_RB);
    const int ns = (K + 3) / 4;
    const double* src[LOCO_RB];
    int64_t pos[LOCO_RB], row[LOCO_RB];
    bool valid[LOCO_RB];
#pragma unroll
    for (int r = 0; r < LOCO_RB; ++r) {
        pos[r] = p0 + 16 * r + e;
        valid[r] = pos[r] < npos;
        row[r] = valid[r] ? idx[pos[r]] : 0;
        src[r] = A + row[r] * lda;
    }
    auto ld = [&](int r, int k) -> double { return (valid[r] && k < K) ? src[r][k] : 0.0; };
    double x[LOCO_RB][NS];
    if constexpr (NT > 0) {
#pragma unroll
        for (int r = 0; r < LOCO_RB; ++r)
#pragma unroll
            for (int s = 0; s < NS; ++s) x[r][s] = ld(r, 4 * s + ks);
    }
    // a_i . beta (the order of fsnap_uq.hip's predictive mean), w_i, e_i = w_i b_i - w_i (a_i . beta)
#pragma unroll
    for (int r = 0; r < LOCO_RB; ++r) {
        double p = 0.0;
        if constexpr (NT > 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) p = __builtin_fma(x[r][s], bp[4 * s + ks], p);
        } else {
            for (int s = 0; s < ns; ++s) p = __builtin_fma(ld(r, 4 * s + ks), bp[4 * s + ks], p);
        }
        p = ks_sum(p);
        if (ks == 0 && valid[r]) {
            const double w = wpack[2 * row[r]], wb = wpack[2 * row[r] + 1];
            pb[pos[r]] = p;
            pw[pos[r]] = w;
            pe[pos[r]] = wb - w * p;
        }
    }
    const int njt = Jp / 16;
    for (int jt = 0; jt < njt; ++jt) {
        d4 acc[LOCO_RB];
#pragma unroll
        for (int r = 0; r < LOCO_RB; ++r) acc[r] = d4{0.0, 0.0, 0.0, 0.0};
        const double* mcol = Mp + 16 * jt + e;
        if constexpr (NT > 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double mf = mcol[(int64_t)(4 * s + ks) * Jp];
#pragma unroll
                for (int r = 0; r < LOCO_RB; ++r) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(mf, x[r][s], acc[r], 0, 0, 0);
            }
        } else {
            for (int s = 0; s < ns; ++s) {
                const double mf = mcol[(int64_t)(4 * s + ks) * Jp];
#pragma unroll
                for (int r = 0; r < LOCO_RB; ++r)
                    acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(mf, ld(r, 4 * s + ks), acc[r], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < LOCO_RB; ++r) {
            if (!valid[r]) continue;
            double* dst = Z + pos[r] * Jp + 16 * jt + ks;
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[4 * g] = acc[r][g];
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void fsnap_loco_cfg_k(const double* __restrict__ Z, int Jp, int J,
                                                        const double* __restrict__ pw, const double* __restrict__ pe,
                                                        const double* __restrict__ pb, const int* __restrict__ idx,
                                                        const int64_t* __restrict__ off, const int* __restrict__ clist,
                                                        int ncl, double* __restrict__ Hg, int dmax, double* __restrict__ vg,
                                                        double* __restrict__ pred, double* __restrict__ info) {
    double* vbuf = vg + (int64_t)blockIdx.x * Jp;
    if constexpr (D > 0) {
        __shared__ double sH[D * D];
        __shared__ double sr[D];
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            loco_one_cfg<false>(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), sH, D, sr, vbuf, pred,
                                info + 4 * (int64_t)c);
        }
    } else {
        double* H = Hg + (int64_t)blockIdx.x * fsnap::loco_scratch_doubles(dmax);
        double* r = H + (int64_t)dmax * dmax;
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            loco_one_cfg<false>(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), H, dmax, r, vbuf, pred,
                                info + 4 * (int64_t)c);
        }
    }
}

}  // namespace

namespace fsnap {

hipError_t launch_loco_zeta(const double* A, int64_t lda, int K, const int* idx, int64_t npos, const double* wpack,
                            const double* Mp, int Jp, const double* bp, double* Z, double* pw, double* pe, double* pb,
                            hipStream_t st) {
    if (npos <= 0) return hipSuccess;
    const int64_t per_block = 4 * 16 * LOCO_RB;
    const dim3 grid((unsigned)((npos + per_block - 1) / per_block));
    dispatch_nt((K + 15) / 16, [&](auto nt) {
        fsnap_loco_zeta_k<decltype(nt)::value><<<grid, 256, 0, st>>>(A, lda, K, idx, npos, wpack, Mp, Jp, bp, Z, pw, pe, pb);
    });
    return hipGetLastError();
}

hipError_t launch_loco_cfg(int D, int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                           const double* pb, const int* idx, const int64_t* off, const int* clist, int ncl, double* Hg,
                           int dmax, double* vg, double* pred, double* info, hipStream_t st) {
    if (ncl <= 0 || nblocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)nblocks);
    const bool known = dispatch_d(D, [&](auto dd) {
        fsnap_loco_cfg_k<decltype(dd)::value><<<grid, 256, 0, st>>>(Z, Jp, J, pw, pe, pb, idx, off, clist, ncl, Hg, dmax, vg, pred, info);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace fsnap
