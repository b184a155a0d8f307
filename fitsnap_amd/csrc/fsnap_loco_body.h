// fsnap_loco_body.h — the per-configuration body of the leave-one-configuration-out kernels: kernel L2 of fsnap_loco.hip
// (UQ = false) and kernel L3 of fsnap_loco_uq.hip (UQ = true) run the same statements in the same order, so the LOO
// predictions of the two are bit-identical.  UQ = true only keeps what kernel L3 needs afterwards and changes no value that
// the prediction reads:
//   n space  the unweighted Gram zeta_i . zeta_j goes to the strict upper triangle of H (which the factorisation and the
//            solves never touch) and its diagonal to gd; the upper part of a diagonal tile, where L2 stores H, holds it too
//   J space  a copy of the right-hand side Z_c^T e_c goes to r0
// Internal.
#pragma once
#include "fsnap_device_common.h"
#include "fsnap_kernels.h"

// Kernel L2.  H: d x d (leading dimension ldh) in LDS (D > 0) or in this workgroup's slice of global scratch (D = 0);
// r: d doubles; vbuf: Jp doubles of global scratch per workgroup.
// Returns whether the configuration is identifiable (uniform over the workgroup).  gd, r0: d doubles each (UQ only).
template <bool UQ>
__device__ __forceinline__ bool loco_one_cfg(const double* __restrict__ Z, int Jp, int J, const double* __restrict__ pw,
                                             const double* __restrict__ pe, const double* __restrict__ pb,
                                             const int* __restrict__ idx, int64_t base, int n, double* H, int ldh, double* r,
                                             double* __restrict__ vbuf, double* __restrict__ pred,
                                             double* __restrict__ info_c, double* gd = nullptr, double* r0 = nullptr) {
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
                if constexpr (UQ) {
                    if (nspace) {
                        if (i == j) gd[i] = gv;
                        if (i < j) {                // a diagonal tile computes both halves: bitwise the same Gram entry
                            H[(int64_t)i * ldh + j] = gv;
                            continue;
                        }
                        if (ti != tj) H[(int64_t)j * ldh + i] = gv;
                    }
                }
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
        if constexpr (UQ) r0[a] = s;
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
        return false;
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
    return true;
}
