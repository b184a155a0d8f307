// fsnap_loco_uq.hip — leave-one-configuration-out predictive variances of a linear smoother (gfx950 only).
//
// With the conventions of fsnap_loco.hip (zeta_i = a_i M, z_i = w_i zeta_i, e_i = w_i b_i - w_i a_i . beta, and per
// configuration c of n rows H_c = I - Z_c Z_c^T (n space, n <= J) or I - Z_c^T Z_c (J space) = L L^T), H_c^-1 is the
// predictive covariance of the configuration's weighted rows under the fit without c, in units of the noise.  Per row and
// per configuration:
//     q_i   = a_i (G - X_c^T X_c + alpha I)^-1 a_i^T       the leave-out leverage of the unweighted row
//           = |L^-1 zeta_i^T|^2                                      (J space)
//           = |zeta_i|^2 + |L^-1 g_i|^2,  g_i = Z_c zeta_i^T         (n space; never (H^-1)_ii - 1, which cancels)
//     l_c   = log det H_c = 2 sum_k log L_kk                         (the same number in either space)
//     D_c   = e_c^T H_c^-1 e_c = e_c . u                             (n space, u the solve of kernel L2)
//           = |e_c|^2 + (Z_c^T e_c) . v                              (J space, v the solve of kernel L2)
//
//   L3  fsnap_loco_uq_cfg_k<D>  kernel L2's geometry (one workgroup of 4 waves per configuration, grid-stride over a bin's
//                               list; D = 32 / 64 / 128 in LDS, D = 0 on a slice of global scratch).  Per configuration:
//       1. loco_one_cfg<true> (fsnap_loco_body.h): L2's statements in L2's order -- H on MFMA, the Cholesky with its pivot
//          rule, the solve, p_i -- so the predictions are those of fsnap_loco_cfg_k bit for bit.  In n space it leaves the
//          unweighted Gram in the strict upper triangle of the d x d array, which L (in the lower one) never needs, and
//          the Gram's diagonal in gd; in J space a copy of Z_c^T e_c in r0.
//       2. l_c and D_c: per-thread partial sums over k = tid, tid + 256, ... in that order, then a binary tree over the 256
//          partials in LDS.
//       3. L is inverted in place, column by column from the last (X_jj = 1 / L_jj, X_ij = -X_jj sum_{j < k <= i} X_ik L_kj),
//          one thread per row i, the new column staged in r so that no thread reads an entry another one has replaced.
//       4. q_i on MFMA: Y = X B with B = zeta^T (J space, from global) or W Gram (n space, from the upper triangle), one
//          wave per 16 right-hand sides, 16 x 16 tiles of Y accumulated over the columns of X up to the diagonal tile,
//          squared and summed per lane over the register index and the tile row, then over the 4 k-slot lanes (ks_sum).
// The LDS array has leading dimension D + 1: the row reads of step 3 and the A operand of step 4 would otherwise hit one
// bank 16 to 32 times (D = 128: 134 KiB of the CU's 160).  Every sum runs in an order that depends on the configuration's own rows
// alone: results are bit-identical run to run and under any permutation or subset of the configurations.  fp64 only, no
// atomics; results are written with plain vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_loco_body.h"
#include "fsnap_wave_sum.h"

namespace {

// sum of f(k), k = 0 ... count - 1: thread t adds k = t, t + 256, ... in order into part[t], then a binary tree over the 256
// partials (part[t] += part[t + 128], ... + 64, ..., + 1): a fixed order, and pairwise like the host's sums rather than one
// chain of 256.  Every thread returns the total.  part: 256 doubles of LDS.
template <class F>
__device__ __forceinline__ double block_sum_fixed(int count, double* part, F&& f) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int k = tid; k < count; k += 256) s += f(k);
    part[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    const double total = part[0];
    __syncthreads();    // part is reused by the next sum
    return total;
}

// H, r, r0, gd as loco_one_cfg<true> takes them; part: 256 doubles of LDS; info_c: 6 doubles.
__device__ __forceinline__ void loco_uq_one_cfg(const double* __restrict__ Z, int Jp, int J, const double* __restrict__ pw,
                                                const double* __restrict__ pe, const double* __restrict__ pb,
                                                const int* __restrict__ idx, int64_t base, int n, double* H, int ldh,
                                                double* r, double* r0, double* gd, double* part, double* __restrict__ vbuf,
                                                double* __restrict__ pred, double* __restrict__ lev,
                                                double* __restrict__ info_c) {
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, ks = lane >> 4, wave = tid >> 6;
    const bool nspace = n <= J;
    const int d = nspace ? n : J;
    const bool ok = loco_one_cfg<true>(Z, Jp, J, pw, pe, pb, idx, base, n, H, ldh, r, vbuf, pred, info_c, gd, r0);
    if (!ok) {
        for (int i = tid; i < n; i += 256) lev[idx[base + i]] = __builtin_nan("");
        if (tid == 0) info_c[4] = info_c[5] = __builtin_nan("");
        return;
    }
    // ---- l_c = 2 sum log L_kk; D_c = e . u (n space) or |e|^2 + (Z^T e) . v (J space) --------------------------------------
    const double logdet = 2.0 * block_sum_fixed(d, part, [&](int k) { return log(H[(int64_t)k * ldh + k]); });
    double dist;
    if (nspace) {
        dist = block_sum_fixed(d, part, [&](int k) { return pe[base + k] * r[k]; });
    } else {
        const double ee = block_sum_fixed(n, part, [&](int i) { return pe[base + i] * pe[base + i]; });
        dist = ee + block_sum_fixed(d, part, [&](int k) { return r0[k] * r[k]; });
    }
    if (tid == 0) {
        info_c[4] = logdet;
        info_c[5] = dist;
    }
    // ---- X = L^-1 in place (lower), columns from the last; r stages the new column (its solve has been used above) --------
    for (int j = d - 1; j >= 0; --j) {
        const double xjj = 1.0 / H[(int64_t)j * ldh + j];
        for (int i = j + 1 + tid; i < d; i += 256) {
            const double* xi = H + (int64_t)i * ldh;
            double s = 0.0;
            for (int k = j + 1; k <= i; ++k) s = __builtin_fma(xi[k], H[(int64_t)k * ldh + j], s);
            r[i] = -(xjj * s);
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < d; i += 256) H[(int64_t)i * ldh + j] = r[i];
        if (tid == 0) H[(int64_t)j * ldh + j] = xjj;
        __syncthreads();
    }
    // ---- q_i = (n space: Gram_ii +) sum_k (X B)_ki^2, B = zeta^T or W Gram ----------------------------------------------------
    const double* Zc = Z + base * Jp;
    const int nt = (d + 15) / 16;
    for (int it = wave; it < (n + 15) / 16; it += 4) {
        const int i = 16 * it + e;
        const bool vi = i < n;
        const double* zi = Zc + (int64_t)(vi ? i : 0) * Jp;
        double q = 0.0;
        for (int kt = 0; kt < nt; ++kt) {
            // A operand lane (e, ks): X[16 kt + e][4 s + ks], zero above the diagonal; B operand: B[4 s + ks][16 it + e]
            const int row = 16 * kt + e;
            const double* xr = H + (int64_t)(row < d ? row : 0) * ldh;
            const int send = 4 * (kt + 1) < (d + 3) / 4 ? 4 * (kt + 1) : (d + 3) / 4;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < send; ++s) {
                const int j = 4 * s + ks;
                const double xa = (row < d && j <= row) ? xr[j] : 0.0;
                double xb = 0.0;
                if (vi && j < d) {
                    if (nspace) {
                        const int lo = i < j ? i : j, hi = i < j ? j : i;
                        xb = pw[base + j] * (lo == hi ? gd[lo] : H[(int64_t)lo * ldh + hi]);
                    } else {
                        xb = zi[j];
                    }
                }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
            }
            // D[reg g] at lane (e, ks) = Y[16 kt + ks + 4 g][16 it + e]
#pragma unroll
            for (int g = 0; g < 4; ++g) q = __builtin_fma(acc[g], acc[g], q);
        }
        q = ks_sum(q);
        if (ks == 0 && vi) lev[idx[base + i]] = nspace ? gd[i] + q : q;
    }
    __syncthreads();    // H, r, gd are reused by the next configuration of this workgroup
}

template <int D>
__global__ __launch_bounds__(256) void fsnap_loco_uq_cfg_k(const double* __restrict__ Z, int Jp, int J,
                                                           const double* __restrict__ pw, const double* __restrict__ pe,
                                                           const double* __restrict__ pb, const int* __restrict__ idx,
                                                           const int64_t* __restrict__ off, const int* __restrict__ clist,
                                                           int ncl, double* __restrict__ Hg, int dmax,
                                                           double* __restrict__ vg, double* __restrict__ pred,
                                                           double* __restrict__ lev, double* __restrict__ info) {
    double* vbuf = vg + (int64_t)blockIdx.x * Jp;
    __shared__ double spart[256];
    if constexpr (D > 0) {
        __shared__ double sH[D * (D + 1)];
        __shared__ double sr[3 * D];
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            loco_uq_one_cfg(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), sH, D + 1, sr, sr + D, sr + 2 * D,
                            spart, vbuf, pred, lev, info + 6 * (int64_t)c);
        }
    } else {
        double* H = Hg + (int64_t)blockIdx.x * fsnap::loco_uq_scratch_doubles(dmax);
        double* r = H + (int64_t)dmax * dmax;
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int c = clist[q];
            loco_uq_one_cfg(Z, Jp, J, pw, pe, pb, idx, off[c], (int)(off[c + 1] - off[c]), H, dmax, r, r + dmax, r + 2 * dmax,
                            spart, vbuf, pred, lev, info + 6 * (int64_t)c);
        }
    }
}

}  // namespace

namespace fsnap {

hipError_t launch_loco_uq_cfg(int D, int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                              const double* pb, const int* idx, const int64_t* off, const int* clist, int ncl, double* Hg,
                              int dmax, double* vg, double* pred, double* lev, double* info, hipStream_t st) {
    if (ncl <= 0 || nblocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)nblocks);
    const bool known = dispatch_d(D, [&](auto dd) {
        fsnap_loco_uq_cfg_k<decltype(dd)::value><<<grid, 256, 0, st>>>(Z, Jp, J, pw, pe, pb, idx, off, clist, ncl, Hg, dmax, vg, pred, lev, info);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace fsnap
