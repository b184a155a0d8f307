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
//                               a slice of global scratch per workgroup (d_c > 128, untuned).
// A configuration whose smallest pivot is <= LOCO_PIVOT_TOL (lambda_max(S_c) -> 1: not identifiable without itself) is
// never divided through: its rows get NaN and its info record says so.  Every sum runs in a fixed order that depends on the
// configuration's own rows only (zeta_i on a_i and M alone, as in fsnap_uq.hip), so a row's result is bit-identical under
// repeats and under any permutation of the configurations.  No atomics; results are written with vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
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

// Kernel L2.  H: d x d (leading dimension ldh) in LDS (D > 0) or in this workgroup's slice of global scratch (D = 0);
// r: d doubles; vbuf: Jp doubles of global scratch per workgroup.
__device__ __forceinline__ void loco_one_cfg(const double* __restrict__ Z, int Jp, int J, const double* __restrict__ pw,
                                             const double* __restrict__ pe, const double* __restrict__ pb,
                                             const int* __restrict__ idx, int64_t base, int n, double* H, int ldh, double* r,
                                             double* __restrict__ vbuf, double* __restrict__ pred,
                                             double* __restrict__ info_c) {
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, ks = lane >> 4, wave = tid >> 6;
    const bool nspace = n <= J;
    const int d = nspace ? n : J;
    const int nt = (d + 15) / 16;
    const int ntiles = nt * (nt + 1) / 2;
    const double* Zc = Z + base * Jp;
    // ---- H = I - Z_c Z_c^T (n space) or I - Z_c^T Z_c (J space), lower 16 x 16 tiles -------------------------------------
    for (int t = wave; t < ntiles; t += 4) {
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        const int tj = t - ti * (ti + 1) / 2;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        if (nspace) {
            // A operand lane (e, ks): zeta_{16 ti + e}[4 s + ks]; B operand: zeta_{16 tj + e}[4 s + ks]; unweighted Gram
            const int ia = 16 * ti + e, ib = 16 * tj + e;
            const double* za = Zc + (int64_t)(ia < n ? ia : 0) * Jp;
            const double* zb = Zc + (int64_t)(ib < n ? ib : 0) * Jp;
            const bool va = ia < n, vb = ib < n;
            for (int s = 0; s < Jp / 4; ++s) {
                const double xa = va ? za[4 * s + ks] : 0.0;
                const double xb = vb ? zb[4 * s + ks] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
            }
        } else {
            // A operand lane (e, ks): z_{4 s + ks}[16 ti + e]; B operand: z_{4 s + ks}[16 tj + e]   (z = w zeta)
            const int ca = 16 * ti + e, cb = 16 * tj + e;
            for (int s = 0; s < (n + 3) / 4; ++s) {
                const int i = 4 * s + ks;
                double xa = 0.0, xb = 0.0;
                if (i < n) {
                    const double w = pw[base + i];
                    xa = w * Zc[(int64_t)i * Jp + ca];
                    xb = w * Zc[(int64_t)i * Jp + cb];
                }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
            }
        }
        // D[reg g] at lane (e, ks) = Gram[16 ti + ks + 4 g][16 tj + e]
        const int j = 16 * tj + e;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = 16 * ti + ks + 4 * g;
            if (i < d && j < d) {
                double gv = acc[g];
                if (nspace) gv = (pw[base + i] * pw[base + j]) * gv;
                H[(int64_t)i * ldh + j] = (i == j ? 1.0 : 0.0) - gv;
            }
        }
    }
    // ---- right-hand side: e_c (n space) or Z_c^T e_c (J space) -----------------------------------------------------------
    for (int a = tid; a < d; a += 256) {
        double s = 0.0;
        if (nspace) {
            s = pe[base + a];
        } else {
#pragma unroll 8
            for (int i = 0; i < n; ++i) s = __builtin_fma(pw[base + i] * Zc[(int64_t)i * Jp + a], pe[base + i], s);
        }
        r[a] = s;
    }
    __syncthreads();
    // ---- Cholesky H = L L^T in place (lower), right-looking, pivot check ------------------------------------------------
    double minpiv = __builtin_inf();
    bool ok = true;
    for (int k = 0; k < d; ++k) {
        const double piv = H[(int64_t)k * ldh + k];
        if (!(piv > fsnap::LOCO_PIVOT_TOL)) {     // NaN included; every thread reads the same value: a uniform exit
            minpiv = piv < minpiv ? piv : minpiv;
            ok = false;
            break;
        }
        minpiv = piv < minpiv ? piv : minpiv;
        const double l = __builtin_sqrt(piv);
        __syncthreads();
        for (int i = k + 1 + tid; i < d; i += 256) H[(int64_t)i * ldh + k] = H[(int64_t)i * ldh + k] / l;
        if (tid == 0) H[(int64_t)k * ldh + k] = l;
        __syncthreads();
        // trailing lower triangle: a 16 x 16 thread grid strides over rows (ty) and columns (tx)
        for (int i = k + 1 + (tid >> 4); i < d; i += 16) {
            const double lik = H[(int64_t)i * ldh + k];
            for (int j = k + 1 + (tid & 15); j <= i; j += 16)
                H[(int64_t)i * ldh + j] = __builtin_fma(-lik, H[(int64_t)j * ldh + k], H[(int64_t)i * ldh + j]);
        }
        __syncthreads();
    }
    if (!ok) {
        for (int i = tid; i < n; i += 256) pred[idx[base + i]] = __builtin_nan("");
        if (tid == 0) {
            info_c[0] = d;
            info_c[1] = minpiv;
            info_c[2] = 0.0;
            info_c[3] = nspace ? 1.0 : 0.0;
        }
        __syncthreads();
        return;
    }
    // ---- L y = r, L^T x = y -----------------------------------------------------------------------------------------------
    for (int k = 0; k < d; ++k) {
        if (tid == 0) r[k] = r[k] / H[(int64_t)k * ldh + k];
        __syncthreads();
        const double rk = r[k];
        for (int i = k + 1 + tid; i < d; i += 256) r[i] = __builtin_fma(-H[(int64_t)i * ldh + k], rk, r[i]);
        __syncthreads();
    }
    for (int k = d - 1; k >= 0; --k) {
        if (tid == 0) r[k] = r[k] / H[(int64_t)k * ldh + k];
        __syncthreads();
        const double rk = r[k];
        for (int i = tid; i < k; i += 256) r[i] = __builtin_fma(-H[(int64_t)k * ldh + i], rk, r[i]);
        __syncthreads();
    }
    // ---- v = Z_c^T u (n space) or the solution itself (J space) ----------------------------------------------------------
    const double* v = r;
    if (nspace) {
        for (int a = tid; a < J; a += 256) {
            double s = 0.0;
#pragma unroll 8
            for (int i = 0; i < n; ++i) s = __builtin_fma(pw[base + i] * Zc[(int64_t)i * Jp + a], r[i], s);
            vbuf[a] = s;
        }
        __syncthreads();
        v = vbuf;
    }
    // ---- p_i = a_i . beta - zeta_i . v ------------------------------------------------------------------------------------
    for (int i = tid; i < n; i += 256) {
        const double* zi = Zc + (int64_t)i * Jp;
        double s = 0.0;
#pragma unroll 8
        for (int a = 0; a < J; ++a) s = __builtin_fma(zi[a], v[a], s);
        pred[idx[base + i]] = pb[base + i] - s;
    }
    if (tid == 0) {
        info_c[0] = d;
        info_c[1] = minpiv;
        info_c[2] = 1.0;
        info_c[3] = nspace ? 1.0 : 0.0;
    }
    __syncthreads();    // r, vbuf and H are reused by the next configuration of this workgroup
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
            loco_one_cfg(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), sH, D, sr, vbuf, pred,
                         info + 4 * (int64_t)c);
        }
    } else {
        double* H = Hg + (int64_t)blockIdx.x * ((int64_t)dmax * dmax + dmax);
        double* r = H + (int64_t)dmax * dmax;
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            loco_one_cfg(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), H, dmax, r, vbuf, pred,
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
