// fsnap_joint.hip — joint information-gain and variance-reduction scores of units for active learning (gfx950 only).
//
// With the posterior C = M M^T (M: K x J), the noise variance tau of a unit-weight row and, for every unit u (a run of
// positions [off[u], off[u + 1]) of a unit-sorted row index idx), the weighted rows X = diag(omega) A_u (n x K):
//     Z = X M (n x J),   Pi = X (M B) = Z B (n x r)   for a target T = R^T R with B = M^T R^T (J x r)
//     n space (n <= J):  S = I_n + Z Z^T / tau = L L^T      J space (n > J):  S = I_J + Z^T Z / tau = L L^T
//     gain      = 1/2 logdet(I + X C X^T / tau) = sum log L_ii                      (the same in either space: Sylvester)
//     reduction = tr(T C) - tr(T C') = ||L^-1 Pi||_F^2 / tau  (n space)  =  ||B||_F^2 - ||L^-1 B||_F^2  (J space)
// S is the identity plus a PSD matrix: every pivot is >= 1 in exact arithmetic, there is no threshold and no unit that cannot
// be scored (a pivot that is not > 0 means NaN or Inf went in: the unit's scores are NaN).
//
//   J1  fsnap_joint_rows_k<NT>   one pass over the index positions: omega_i a_i [M | M B] (npos x Wp, by position) on
//                                v_mfma_f64_16x16x4f64 with the factor tile as the A operand and the row block as the B operand
//                                (kernel L1's plan, fsnap_loco.hip: D[reg g] at lane (e, ks) is column 16 jt + ks + 4 g of row e).
//                                NT = ceil(K / 16) <= 9 keeps the rows in registers; NT = 0 (K > 144, untuned) re-reads them per
//                                factor tile.
//   J2  fsnap_joint_unit_k<D>    one workgroup (4 waves) per live unit, grid-stride over a list of units whose dim S =
//                                min(n, J) <= D: S is built in LDS on MFMA (16 x 16 lower tiles, one wave per tile), factorised
//                                by a right-looking Cholesky in LDS, the logs of the diagonal are summed in index order, and
//                                the r right-hand sides are substituted forward 16 columns per wave: block row bi of the
//                                solution is Pi_bi - sum_{bj < bi} L_{bi bj} Y_bj on MFMA -- the Y fragments a lane produced
//                                ARE its B operands of the later block rows (rows ks + 4 g of column e), so they stay in
//                                registers (D / 16 x 4 doubles) and neither Pi nor B needs LDS next to the 128 x 128 S --
//                                followed by the 16 x 16 triangular solve with the diagonal tile (16 steps, one shuffle each).
//                                D = 0: the same code with S and the Y fragments in a slice of global scratch per workgroup
//                                (dim S > 128, untuned).
// Every sum runs in a fixed order that depends on the unit's own rows (and M, B, tau) only: a unit's scores are bit-identical
// under repeats and under any permutation or subset of the units.  No atomics; results are written with vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace {

constexpr int JOINT_RB = 2;   // 16-position blocks per wave in kernel J1

template <int NT>
__global__ __launch_bounds__(256) void fsnap_joint_rows_k(const double* __restrict__ A, int64_t lda, int K,
                                                          const int* __restrict__ idx, int64_t npos,
                                                          const double* __restrict__ om, const double* __restrict__ Fp, int Wp,
                                                          double* __restrict__ ZP) {
    constexpr int NS = NT > 0 ? 4 * NT : 1;
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * JOINT_RB);
    const int ns = (K + 3) / 4;
    const double* src[JOINT_RB];
    int64_t pos[JOINT_RB];
    double wgt[JOINT_RB];
    bool valid[JOINT_RB];
#pragma unroll
    for (int r = 0; r < JOINT_RB; ++r) {
        pos[r] = p0 + 16 * r + e;
        valid[r] = pos[r] < npos;
        src[r] = A + (int64_t)(valid[r] ? idx[pos[r]] : 0) * lda;
        wgt[r] = valid[r] ? om[pos[r]] : 0.0;
    }
    auto ld = [&](int r, int k) -> double { return (valid[r] && k < K) ? src[r][k] : 0.0; };
    double x[JOINT_RB][NS];
    if constexpr (NT > 0) {
#pragma unroll
        for (int r = 0; r < JOINT_RB; ++r)
#pragma unroll
            for (int s = 0; s < NS; ++s) x[r][s] = ld(r, 4 * s + ks);
    }
    const int njt = Wp / 16;
    for (int jt = 0; jt < njt; ++jt) {
        d4 acc[JOINT_RB];
#pragma unroll
        for (int r = 0; r < JOINT_RB; ++r) acc[r] = d4{0.0, 0.0, 0.0, 0.0};
        const double* fcol = Fp + 16 * jt + e;
        if constexpr (NT > 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double ff = fcol[(int64_t)(4 * s + ks) * Wp];
#pragma unroll
                for (int r = 0; r < JOINT_RB; ++r) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(ff, x[r][s], acc[r], 0, 0, 0);
            }
        } else {
            for (int s = 0; s < ns; ++s) {
                const double ff = fcol[(int64_t)(4 * s + ks) * Wp];
#pragma unroll
                for (int r = 0; r < JOINT_RB; ++r)
                    acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(ff, ld(r, 4 * s + ks), acc[r], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < JOINT_RB; ++r) {
            if (!valid[r]) continue;
            double* dst = ZP + pos[r] * Wp + 16 * jt + ks;
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[4 * g] = wgt[r] * acc[r][g];
        }
    }
}

// Forward substitution L Y = RHS for the rp (a multiple of 16) columns of rhs (element (i, c) at rhs[i * ldr + c], rows
// i < d), 16 columns per wave.  NTD > 0: the Y fragments in registers (d <= 16 NTD); NTD = 0: in yw (this wave's
// 4 nt x 64 doubles of scratch, every lane reads back only what it wrote).  Returns this lane's share of the sum of squares of
// the right-hand sides (sb) and of the solution (sy).
template <int NTD>
__device__ __forceinline__ void joint_subst(const double* H, int ldh, int d, const double* __restrict__ rhs, int64_t ldr,
                                            int rp, double* __restrict__ yw, double& sb, double& sy) {
    constexpr int NY = NTD > 0 ? NTD : 1;
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int nt = (d + 15) / 16;
    double yr[NY][4];
    sb = 0.0;
    sy = 0.0;
    auto lfrag = [&](int bi, int bj, int s) -> double {      // A operand: L[16 bi + e][16 bj + 4 s + ks]
        const int i = 16 * bi + e, j = 16 * bj + 4 * s + ks;
        return (i < d && j < d) ? H[(int64_t)i * ldh + j] : 0.0;
    };
    auto diag_solve = [&](int bi, double (&t)[4]) {
        // 16 x 16 lower-triangular solve with the diagonal tile: row i of the tile lives in reg i / 4 of the lanes ks = i % 4
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int gi = i >> 2, ki = i & 3, row = 16 * bi + i;
            double yi = row < d ? t[gi] / H[(int64_t)row * ldh + row] : 0.0;
            yi = __shfl(yi, e + 16 * ki, 64);
            if (ks == ki) t[gi] = yi;
#pragma unroll
            for (int g = gi; g < 4; ++g) {
                const int rr = ks + 4 * g;                  // this lane's row of the tile in reg g
                if (rr > i && 16 * bi + rr < d) t[g] = __builtin_fma(-H[(int64_t)(16 * bi + rr) * ldh + row], yi, t[g]);
            }
        }
    };
    for (int p = wave; p < rp / 16; p += 4) {
        const int col = 16 * p + e;
        if constexpr (NTD > 0) {
#pragma unroll
            for (int bi = 0; bi < NTD; ++bi) {
                if (bi < nt) {
                    double t[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int row = 16 * bi + ks + 4 * g;
                        t[g] = row < d ? rhs[(int64_t)row * ldr + col] : 0.0;
                        sb = __builtin_fma(t[g], t[g], sb);
                    }
                    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int bj = 0; bj < bi; ++bj)
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(lfrag(bi, bj, s), yr[bj][s], acc, 0, 0, 0);
#pragma unroll
                    for (int g = 0; g < 4; ++g) t[g] -= acc[g];
                    diag_solve(bi, t);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        yr[bi][g] = t[g];
                        sy = __builtin_fma(t[g], t[g], sy);
                    }
                }
            }
        } else {
            for (int bi = 0; bi < nt; ++bi) {
                double t[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = 16 * bi + ks + 4 * g;
                    t[g] = row < d ? rhs[(int64_t)row * ldr + col] : 0.0;
                    sb = __builtin_fma(t[g], t[g], sb);
                }
                d4 acc = {0.0, 0.0, 0.0, 0.0};
                for (int bj = 0; bj < bi; ++bj)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(lfrag(bi, bj, s), yw[(4 * bj + s) * 64 + lane], acc, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) t[g] -= acc[g];
                diag_solve(bi, t);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    yw[(4 * bi + g) * 64 + lane] = t[g];
                    sy = __builtin_fma(t[g], t[g], sy);
                }
            }
        }
    }
}

// Kernel J2 for one unit.  H: d x d (leading dimension ldh) in LDS (NTD > 0) or in this workgroup's slice of global scratch;
// lg: d doubles next to it; ws: 4 doubles of LDS; yg: this workgroup's scratch of Y fragments (NTD = 0 only).
template <int NTD>
__device__ __forceinline__ void joint_one_unit(const double* __restrict__ ZP, int Wp, int Jp, int J, int rp,
                                               const double* __restrict__ Bp, double tau, int64_t base, int n, double* H, int ldh,
                                               double* lg, double* ws, double* __restrict__ yg, int ntmax,
                                               double* __restrict__ out_u, double* __restrict__ info_u) {
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, ks = lane >> 4, wave = tid >> 6;
    const bool nspace = n <= J;
    const int d = nspace ? n : J;
    const int nt = (d + 15) / 16;
    const int ntiles = nt * (nt + 1) / 2;
    const double* Zu = ZP + base * Wp;
    // ---- S = I + Z Z^T / tau (n space) or I + Z^T Z / tau (J space), lower 16 x 16 tiles ----------------------------------
    for (int t = wave; t < ntiles; t += 4) {
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        const int tj = t - ti * (ti + 1) / 2;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        if (nspace) {
            const int ia = 16 * ti + e, ib = 16 * tj + e;
            const bool va = ia < n, vb = ib < n;
            const double* za = Zu + (int64_t)(va ? ia : 0) * Wp;
            const double* zb = Zu + (int64_t)(vb ? ib : 0) * Wp;
            for (int s = 0; s < Jp / 4; ++s) {
                const double xa = va ? za[4 * s + ks] : 0.0;
                const double xb = vb ? zb[4 * s + ks] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
            }
        } else {
            const int ca = 16 * ti + e, cb = 16 * tj + e;        // < Jp: the padding columns of Z are zero
            for (int s = 0; s < (n + 3) / 4; ++s) {
                const int i = 4 * s + ks;
                double xa = 0.0, xb = 0.0;
                if (i < n) {
                    xa = Zu[(int64_t)i * Wp + ca];
                    xb = Zu[(int64_t)i * Wp + cb];
                }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
            }
        }
        const int j = 16 * tj + e;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = 16 * ti + ks + 4 * g;
            if (i < d && j < d) H[(int64_t)i * ldh + j] = (i == j ? 1.0 : 0.0) + acc[g] / tau;
        }
    }
    __syncthreads();
    // ---- Cholesky S = L L^T in place (lower), right-looking -----------------------------------------------------------------
    double minpiv = __builtin_inf();
    bool ok = true;
    for (int k = 0; k < d; ++k) {
        const double piv = H[(int64_t)k * ldh + k];
        if (!(piv > 0.0) || piv == __builtin_inf()) {     // NaN included; every thread reads the same value: a uniform exit
            ok = false;
            break;
        }
        minpiv = piv < minpiv ? piv : minpiv;
        const double l = __builtin_sqrt(piv);
        __syncthreads();
        for (int i = k + 1 + tid; i < d; i += 256) H[(int64_t)i * ldh + k] = H[(int64_t)i * ldh + k] / l;
        if (tid == 0) H[(int64_t)k * ldh + k] = l;
        __syncthreads();
        for (int i = k + 1 + (tid >> 4); i < d; i += 16) {
            const double lik = H[(int64_t)i * ldh + k];
            for (int j = k + 1 + (tid & 15); j <= i; j += 16)
                H[(int64_t)i * ldh + j] = __builtin_fma(-lik, H[(int64_t)j * ldh + k], H[(int64_t)i * ldh + j]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        info_u[0] = d;
        info_u[1] = nspace ? 1.0 : 0.0;
        info_u[2] = ok ? minpiv : __builtin_nan("");
        info_u[3] = n;
    }
    if (!ok) {
        if (tid == 0) {
            out_u[0] = __builtin_nan("");
            out_u[1] = __builtin_nan("");
        }
        __syncthreads();
        return;
    }
    // ---- gain = sum log L_ii, in index order --------------------------------------------------------------------------------
    for (int i = tid; i < d; i += 256) lg[i] = log(H[(int64_t)i * ldh + i]);
    // ---- reduction: forward substitution of the r right-hand sides ----------------------------------------------------------
    double part = 0.0;
    if (rp > 0) {
        double sb, sy;
        const double* rhs = nspace ? Zu + Jp : Bp;
        joint_subst<NTD>(H, ldh, d, rhs, nspace ? Wp : rp, rp, yg + (int64_t)wave * (4 * ntmax * 64), sb, sy);
        part = wave_sum(nspace ? sy : sb - sy);
    }
    if (lane == 0) ws[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s += lg[i];
        out_u[0] = s;
        const double red = ((ws[0] + ws[1]) + ws[2]) + ws[3];
        out_u[1] = rp > 0 ? (nspace ? red / tau : red) : __builtin_nan("");
    }
    __syncthreads();    // H, lg and ws are reused by the next unit of this workgroup
}

template <int D>
__global__ __launch_bounds__(256) void fsnap_joint_unit_k(const double* __restrict__ ZP, int Wp, int Jp, int J, int rp,
                                                          const double* __restrict__ Bp, double tau,
                                                          const int64_t* __restrict__ off, const int* __restrict__ ulist, int ncl,
                                                          double* __restrict__ Sg, int dmax, double* __restrict__ Yg,
                                                          double* __restrict__ out, double* __restrict__ info) {
    __shared__ double ws[4];
    if constexpr (D > 0) {
        constexpr int LDH = D + 2;      // rows 4 banks apart: the 16 rows x 2 k of half a wave's MFMA operand read hit 32 banks
        __shared__ double sH[D * LDH];
        __shared__ double slg[D];
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int u = ulist[q];
            joint_one_unit<D / 16>(ZP, Wp, Jp, J, rp, Bp, tau, off[u], (int)(off[u + 1] - off[u]), sH, LDH, slg, ws, nullptr, 0,
                                   out + 2 * (int64_t)u, info + 4 * (int64_t)u);
        }
    } else {
        double* H = Sg + (int64_t)blockIdx.x * fsnap::loco_scratch_doubles(dmax);
        double* lg = H + (int64_t)dmax * dmax;
        const int ntmax = (dmax + 15) / 16;
        double* yg = Yg + (int64_t)blockIdx.x * fsnap::joint_yslice(dmax);
        for (int q = blockIdx.x; q < ncl; q += gridDim.x) {
            const int u = ulist[q];
            joint_one_unit<0>(ZP, Wp, Jp, J, rp, Bp, tau, off[u], (int)(off[u + 1] - off[u]), H, dmax, lg, ws, yg, ntmax,
                              out + 2 * (int64_t)u, info + 4 * (int64_t)u);
        }
    }
}

}  // namespace

namespace fsnap {

hipError_t launch_joint_rows(const double* A, int64_t lda, int K, const int* idx, int64_t npos, const double* om,
                             const double* Fp, int Wp, double* ZP, hipStream_t st) {
    if (npos <= 0) return hipSuccess;
    const int64_t per_block = 4 * 16 * JOINT_RB;
    const dim3 grid((unsigned)((npos + per_block - 1) / per_block));
    dispatch_nt((K + 15) / 16, [&](auto nt) {
        fsnap_joint_rows_k<decltype(nt)::value><<<grid, 256, 0, st>>>(A, lda, K, idx, npos, om, Fp, Wp, ZP);
    });
    return hipGetLastError();
}

hipError_t launch_joint_units(int D, int nblocks, const double* ZP, int Wp, int Jp, int J, int rp, const double* Bp, double tau,
                              const int64_t* off, const int* ulist, int ncl, double* Sg, int dmax, double* Yg, double* out,
                              double* info, hipStream_t st) {
    if (ncl <= 0 || nblocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)nblocks);
    const bool known = dispatch_d(D, [&](auto dd) {
        fsnap_joint_unit_k<decltype(dd)::value><<<grid, 256, 0, st>>>(ZP, Wp, Jp, J, rp, Bp, tau, off, ulist, ncl, Sg, dmax, Yg, out, info);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace fsnap
