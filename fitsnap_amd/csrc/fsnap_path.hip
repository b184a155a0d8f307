// fsnap_path.hip — exact leave-one-unit-out errors of ridge fits over a grid of alphas (gfx950 only, K <= 144).
//
// With the weighted training rows x_i = w_i a_i, y_i = w_i b_i (kernel 1A's wpack: w_i = 0 off the mask) and the statistics
// G = sum x x^T, c = sum x y of the fit, for every unit u (a run of positions [off[u], off[u + 1]) of a unit-sorted row
// index idx) and every grid point alpha_q >= 0 the REFIT without the unit's rows (not the Woodbury form of fsnap_loco.hip):
//     G_u = X_u^T X_u,  c_u = X_u^T y_u                                  once per unit, shared by all alphas
//     B_q = G - G_u + alpha_q I,  D_q = sqrt(diag B_q),  H_q = D_q^-1 B_q D_q^-1      (unit diagonal)
//     beta_q = D_q^-1 H_q^-1 D_q^-1 (c - c_u)                             Cholesky of H_q with a pivot check
//     p_i^q = a_i . beta_q,  r_i^q = b_i - p_i^q                          for every row i of u
//
//   P1  fsnap_path_k<NTMAX>   one workgroup (4 waves) per unit, grid-stride over the units.  K is padded to nt = ceil(K / 16)
//                             tile rows (NTMAX = 2 / 4 / 6 / 9 sizes the LDS only).
//       1. G_u on v_mfma_f64_16x16x4f64, lower 16 x 16 tiles, the unit's weighted rows as both operands (the J-space branch
//          of fsnap_loco.hip's loco_one_cfg on x_i itself); the base G - G_u goes to this workgroup's slice of global scratch
//          by lower tiles (L2-resident: it is read once per alpha, coalesced), c - c_u and the base's diagonal to LDS.
//       2. per alpha: the scaled work copy H_q in LDS by lower tiles (a square 144 x 144 would not fit beside the rest; 45
//          tiles of 16 x 17 doubles do), a right-looking Cholesky in 16-column panels -- the diagonal tile inside wave 0 in
//          registers (shuffles, no barrier), the panel below by substitution (one thread per row), the trailing tiles on
//          MFMA: three barriers per panel -- and the two triangular solves in 16-blocks likewise.  A diagonal entry of B_q
//          that is <= 0 or has cancelled to <= LOCO_PIVOT_TOL (G_jj + alpha_q) (the unit alone touches the column: in
//          floating point the downdate leaves rounding noise of either sign, not 0), or a pivot <= LOCO_PIVOT_TOL, ends the
//          factorisation uniformly: the unit is not identifiable at that alpha, it is never divided through.
//       3. per chunk of 16 alphas: the predictions of the unit's rows for all 16 betas at once on MFMA (betas as the A
//          operand, the rows, re-read from L2, as the B operand), staged through LDS in blocks of 64 rows; thread
//          (q, class) adds n, sum |r|, sum r^2, sum (w r)^2 over the rows of its class in position order.
// Every sum runs in an order that depends on the unit's own rows only: results are bit-identical run to run and under any
// permutation of the units.  No atomics; results are written with vector stores.  Nothing of size O(m K) is written.
#include "fsnap_device_common.h"
#include "fsnap_kernels.h"

namespace {

constexpr int PT_RS = 17;            // row stride of a work tile in LDS (16 + 1: a thread per row reads without bank conflicts)
constexpr int PT_TS = 16 * PT_RS;    // doubles per work tile
constexpr int PT_QC = fsnap::PATH_QCHUNK;
constexpr int PT_RC = 64;            // rows per staged block of predictions

__device__ __forceinline__ int pt_tile(int ti, int tj) { return ti * (ti + 1) / 2 + tj; }

__device__ __forceinline__ void pt_split(int t, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

// Cholesky of one 16 x 16 diagonal tile T (LDS, row stride PT_RS) inside one wave: lane (e, ks) holds T[ks + 4 g][e], g < 4.
// Returns false at the first pivot <= tol (minpiv: the smallest pivot met, that one included).  Only the lower triangle of
// the result is meaningful.
__device__ __forceinline__ bool pt_diag_tile(double* T, int e, int ks, double& minpiv) {
    double t[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) t[g] = T[(ks + 4 * g) * PT_RS + e];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (ok) {                                           // wave-uniform
            const double piv = __shfl(t[k >> 2], k + 16 * (k & 3), 64);
            minpiv = piv < minpiv ? piv : minpiv;
            if (!(piv > fsnap::LOCO_PIVOT_TOL)) {           // NaN included
                minpiv = piv == piv ? minpiv : piv;
                ok = false;
            } else {
                const double l = __builtin_sqrt(piv);
                if (e == k) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int row = ks + 4 * g;
                        if (row > k) t[g] = t[g] / l;
                        else if (row == k) t[g] = l;
                    }
                }
                double lik[4], ljk4[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    lik[g] = __shfl(t[g], k + 16 * ks, 64);          // L[ks + 4 g][k]
                    ljk4[g] = __shfl(t[g], k + 16 * (e & 3), 64);    // L[(e & 3) + 4 g][k]
                }
                const int eg = e >> 2;
                const double ljk = eg == 0 ? ljk4[0] : eg == 1 ? ljk4[1] : eg == 2 ? ljk4[2] : ljk4[3];   // L[e][k]
                if (e > k) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (ks + 4 * g > k) t[g] = __builtin_fma(-lik[g], ljk, t[g]);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) T[(ks + 4 * g) * PT_RS + e] = t[g];
    return ok;
}

struct PathArgs {
    const double* A;
    int64_t lda;
    int K;
    const double* wpack;
    const double* b;
    const int* idx;
    const int64_t* off;
    int nunits;
    const double* G;
    const double* c;
    const double* alphas;
    int Q;
    const unsigned char* rcls;
    int nclass;
    double* Bg;
    double* sums;
    double* info;
    double* pred;
    int64_t m;
};

template <int NTMAX>
__global__ __launch_bounds__(256) void fsnap_path_k(const PathArgs a) {
    constexpr int NTILES = NTMAX * (NTMAX + 1) / 2;
    constexpr int KPMAX = 16 * NTMAX;
    __shared__ double sW[NTILES * PT_TS];
    __shared__ double sBeta[PT_QC * (KPMAX + 1)];
    __shared__ double sStage[PT_RC * PT_RS];
    __shared__ double sR[KPMAX], sBd[KPMAX], sDinv[KPMAX], sY[KPMAX];
    __shared__ double sRb[PT_RC], sRw[PT_RC];
    __shared__ int sRc[PT_RC];
    __shared__ int sOk[PT_QC];
    __shared__ int sMap[NTILES];
    __shared__ double sPiv;
    __shared__ int sFlag;

    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, ks = lane >> 4, wave = tid >> 6;
    const int K = a.K, nt = (K + 15) / 16, Kp = 16 * nt, ntiles = nt * (nt + 1) / 2, BS = Kp + 1;
    double* Bt = a.Bg + (int64_t)blockIdx.x * ntiles * 256;
    for (int t = tid; t < ntiles; t += 256) {
        int ti, tj;
        pt_split(t, ti, tj);
        sMap[t] = ti | (tj << 8);
    }
    __syncthreads();

    for (int u = blockIdx.x; u < a.nunits; u += gridDim.x) {
        const int64_t base = a.off[u];
        const int n = (int)(a.off[u + 1] - base);
        if (n == 0) {                                             // nothing to leave out: zero sums, info (inf, 1)
            for (int x = tid; x < a.Q * a.nclass * 4; x += 256) {
                const int q = x / (a.nclass * 4), r = x - q * a.nclass * 4;
                a.sums[4 * ((int64_t)q * a.nunits + u) * a.nclass + r] = 0.0;
            }
            for (int q = tid; q < a.Q; q += 256) {
                a.info[2 * ((int64_t)q * a.nunits + u)] = __builtin_inf();
                a.info[2 * ((int64_t)q * a.nunits + u) + 1] = 1.0;
            }
            continue;
        }
        // ---- 1. base = G - G_u by lower tiles (global scratch), r = c - c_u, the base's diagonal --------------------------
        for (int t = wave; t < ntiles; t += 4) {
            const int ti = sMap[t] & 255, tj = sMap[t] >> 8;
            const int ca = 16 * ti + e, cb = 16 * tj + e;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < (n + 3) / 4; ++s) {
                const int i = 4 * s + ks;
                double xa = 0.0, xb = 0.0;
                if (i < n) {
                    const int64_t row = a.idx[base + i];
                    const double w = a.wpack[2 * row];
                    const double* ar = a.A + row * a.lda;
                    if (ca < K) xa = w * ar[ca];
                    if (cb < K) xb = w * ar[cb];
                }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, acc, 0, 0, 0);
            }
            // D[reg g] at lane (e, ks) = G_u[16 ti + ks + 4 g][16 tj + e]
            const int j = 16 * tj + e;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = 16 * ti + ks + 4 * g;
                Bt[t * 256 + (ks + 4 * g) * 16 + e] = (i < K && j < K) ? a.G[(int64_t)i * K + j] - acc[g] : 0.0;
            }
        }
        for (int j = tid; j < Kp; j += 256) {
            double s = 0.0;
            if (j < K) {
                double cu = 0.0;
#pragma unroll 8
                for (int i = 0; i < n; ++i) {
                    const int64_t row = a.idx[base + i];
                    cu = __builtin_fma(a.wpack[2 * row] * a.A[row * a.lda + j], a.wpack[2 * row + 1], cu);
                }
                s = a.c[j] - cu;
            }
            sR[j] = s;
        }
        __syncthreads();
        for (int j = tid; j < Kp; j += 256) sBd[j] = j < K ? Bt[pt_tile(j >> 4, j >> 4) * 256 + (j & 15) * 17] : 0.0;

        double cnt = 0.0, sabs = 0.0, ssq = 0.0, swsq = 0.0;     // thread (q = tid & 15, class = tid >> 4), tid < 128
        for (int q0 = 0; q0 < a.Q; q0 += PT_QC) {
            const int qc = a.Q - q0 < PT_QC ? a.Q - q0 : PT_QC;
            for (int ql = 0; ql < PT_QC; ++ql) {
                if (ql >= qc) {                                   // unused slots of the last chunk: zero betas
                    for (int j = tid; j < Kp; j += 256) sBeta[ql * BS + j] = 0.0;
                    if (tid == 0) sOk[ql] = 0;
                    continue;
                }
                const double alpha = a.alphas[q0 + ql];
                double* info_q = a.info + 2 * ((int64_t)(q0 + ql) * a.nunits + u);
                // ---- 2a. scaling ----------------------------------------------------------------------------------------
                __syncthreads();                                  // sBd written; sY, sW of the alpha before are free
                int bad = 0;
                for (int j = tid; j < Kp; j += 256) {
                    const double dj = j < K ? sBd[j] + alpha : 1.0;
                    const double gj = j < K ? a.G[(int64_t)j * K + j] + alpha : 1.0;
                    bad |= !(dj > fsnap::LOCO_PIVOT_TOL * gj) || !(dj > 0.0);
                    sDinv[j] = dj > 0.0 ? 1.0 / __builtin_sqrt(dj) : 0.0;
                }
                bad = __syncthreads_or(bad);
                if (bad) {                                        // a diagonal entry of B_q cancelled: not identifiable
                    for (int j = tid; j < Kp; j += 256) sBeta[ql * BS + j] = __builtin_nan("");
                    if (tid == 0) {
                        double mn = __builtin_inf();
                        for (int j = 0; j < K; ++j) {
                            const double dj = sBd[j] + alpha;
                            mn = (dj < mn || dj != dj) ? dj : mn;
                        }
                        info_q[0] = mn;
                        info_q[1] = 0.0;
                        sOk[ql] = 0;
                    }
                    continue;
                }
                for (int x = tid; x < ntiles * 256; x += 256) {
                    const int t = x >> 8, r = (x >> 4) & 15, cc = x & 15;
                    const int i = 16 * (sMap[t] & 255) + r, j = 16 * (sMap[t] >> 8) + cc;
                    sW[t * PT_TS + r * PT_RS + cc] = i == j ? 1.0 : Bt[x] * sDinv[i] * sDinv[j];
                }
                for (int j = tid; j < Kp; j += 256) sY[j] = sR[j] * sDinv[j];
                __syncthreads();
                // ---- 2b. blocked Cholesky H = L L^T in place (lower tiles) ---------------------------------------------
                double minpiv = __builtin_inf();
                bool ok = true;
                for (int p = 0; p < nt; ++p) {
                    double* Lpp = sW + pt_tile(p, p) * PT_TS;
                    if (wave == 0) {
                        double mp = __builtin_inf();
                        const bool okp = pt_diag_tile(Lpp, e, ks, mp);
                        if (lane == 0) {
                            sPiv = mp;
                            sFlag = okp ? 1 : 0;
                        }
                    }
                    __syncthreads();
                    {
                        const double mp = sPiv;
                        minpiv = (mp < minpiv || mp != mp) ? mp : minpiv;
                    }
                    if (!sFlag) {                                 // every thread reads the same word: a uniform exit
                        ok = false;
                        break;
                    }
                    const int rem = nt - p - 1;
                    if (rem == 0) break;
                    if (tid < 16 * rem) {                         // panel below: X L_pp^T = A, one row per thread
                        double* row = sW + pt_tile(p + 1 + (tid >> 4), p) * PT_TS + (tid & 15) * PT_RS;
                        double x[16];
#pragma unroll
                        for (int cc = 0; cc < 16; ++cc) {
                            double v = row[cc];
#pragma unroll
                            for (int k = 0; k < cc; ++k) v = __builtin_fma(-x[k], Lpp[cc * PT_RS + k], v);
                            x[cc] = v / Lpp[cc * PT_RS + cc];
                        }
#pragma unroll
                        for (int cc = 0; cc < 16; ++cc) row[cc] = x[cc];
                    }
                    __syncthreads();
                    const int ntr = rem * (rem + 1) / 2;          // trailing tiles: W[ti][tj] -= L[ti][p] L[tj][p]^T
                    for (int tt = wave; tt < ntr; tt += 4) {
                        const int ti = p + 1 + (sMap[tt] & 255), tj = p + 1 + (sMap[tt] >> 8);
                        const double* La = sW + pt_tile(ti, p) * PT_TS;
                        const double* Lb = sW + pt_tile(tj, p) * PT_TS;
                        double* Wt = sW + pt_tile(ti, tj) * PT_TS;
                        d4 acc;
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc[g] = Wt[(ks + 4 * g) * PT_RS + e];
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-La[e * PT_RS + 4 * s + ks], Lb[e * PT_RS + 4 * s + ks],
                                                                       acc, 0, 0, 0);
#pragma unroll
                        for (int g = 0; g < 4; ++g) Wt[(ks + 4 * g) * PT_RS + e] = acc[g];
                    }
                    __syncthreads();
                }
                if (!ok) {
                    for (int j = tid; j < Kp; j += 256) sBeta[ql * BS + j] = __builtin_nan("");
                    if (tid == 0) {
                        info_q[0] = minpiv;
                        info_q[1] = 0.0;
                        sOk[ql] = 0;
                    }
                    continue;
                }
                // ---- 2c. L y = D^-1 r, L^T x = y in 16-blocks, beta = D^-1 x -------------------------------------------
                for (int p = 0; p < nt; ++p) {
                    const double* Lpp = sW + pt_tile(p, p) * PT_TS;
                    if (wave == 0) {
                        double v = sY[16 * p + e];
#pragma unroll
                        for (int k = 0; k < 16; ++k) {
                            const double vk = __shfl(v, k, 64) / Lpp[k * PT_RS + k];
                            if (e == k) v = vk;
                            else if (e > k) v = __builtin_fma(-Lpp[e * PT_RS + k], vk, v);
                        }
                        if (ks == 0) sY[16 * p + e] = v;
                    }
                    __syncthreads();
                    const int rem = nt - p - 1;
                    if (tid < 16 * rem) {
                        const double* row = sW + pt_tile(p + 1 + (tid >> 4), p) * PT_TS + (tid & 15) * PT_RS;
                        double s = sY[16 * (p + 1) + tid];
#pragma unroll
                        for (int k = 0; k < 16; ++k) s = __builtin_fma(-row[k], sY[16 * p + k], s);
                        sY[16 * (p + 1) + tid] = s;
                    }
                    __syncthreads();
                }
                for (int p = nt - 1; p >= 0; --p) {
                    const double* Lpp = sW + pt_tile(p, p) * PT_TS;
                    if (wave == 0) {
                        double v = sY[16 * p + e];
#pragma unroll
                        for (int k = 15; k >= 0; --k) {
                            const double vk = __shfl(v, k, 64) / Lpp[k * PT_RS + k];
                            if (e == k) v = vk;
                            else if (e < k) v = __builtin_fma(-Lpp[k * PT_RS + e], vk, v);
                        }
                        if (ks == 0) sY[16 * p + e] = v;
                    }
                    __syncthreads();
                    if (tid < 16 * p) {
                        const double* col = sW + pt_tile(p, tid >> 4) * PT_TS + (tid & 15);
                        double s = sY[tid];
#pragma unroll
                        for (int k = 0; k < 16; ++k) s = __builtin_fma(-col[k * PT_RS], sY[16 * p + k], s);
                        sY[tid] = s;
                    }
                    __syncthreads();
                }
                for (int j = tid; j < Kp; j += 256) sBeta[ql * BS + j] = j < K ? sY[j] * sDinv[j] : 0.0;
                if (tid == 0) {
                    info_q[0] = minpiv;
                    info_q[1] = 1.0;
                    sOk[ql] = 1;
                }
            }
            __syncthreads();
            // ---- 3. predictions of the unit's rows for the chunk's betas, sums per (q, class) ------------------------------
            const int sq = tid & 15, scls = tid >> 4;
            for (int r0 = 0; r0 < n; r0 += PT_RC) {
                const int pos = r0 + 16 * wave + e;
                const bool valid = pos < n;
                const int64_t row = valid ? a.idx[base + pos] : 0;
                const double* ar = a.A + row * a.lda;
                d4 acc = {0.0, 0.0, 0.0, 0.0};
                for (int s = 0; s < Kp / 4; ++s) {
                    const int k = 4 * s + ks;
                    const double xb = (valid && k < K) ? ar[k] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sBeta[e * BS + k], xb, acc, 0, 0, 0);
                }
                // D[reg g] at lane (e, ks) = a_{row e} . beta_{ks + 4 g}
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ql = ks + 4 * g;
                    sStage[(16 * wave + e) * PT_RS + ql] = acc[g];
                    if (a.pred && valid && ql < qc)
                        a.pred[(int64_t)(q0 + ql) * a.m + row] = sOk[ql] ? acc[g] : __builtin_nan("");
                }
                if (ks == 0) {
                    sRb[16 * wave + e] = valid ? a.b[row] : 0.0;
                    sRw[16 * wave + e] = valid ? a.wpack[2 * row] : 0.0;
                    sRc[16 * wave + e] = valid ? (int)a.rcls[row] : -1;
                }
                __syncthreads();
                if (tid < 128 && sq < qc && sOk[sq]) {
                    const int nr = n - r0 < PT_RC ? n - r0 : PT_RC;
                    for (int i = 0; i < nr; ++i) {
                        if (sRc[i] == scls) {
                            const double r = sRb[i] - sStage[i * PT_RS + sq];
                            const double wr = sRw[i] * r;
                            cnt += 1.0;
                            sabs += __builtin_fabs(r);
                            ssq = __builtin_fma(r, r, ssq);
                            swsq = __builtin_fma(wr, wr, swsq);
                        }
                    }
                }
                __syncthreads();
            }
            if (tid < 128 && sq < qc && scls < a.nclass) {
                double* out = a.sums + 4 * (((int64_t)(q0 + sq) * a.nunits + u) * a.nclass + scls);
                out[0] = cnt;
                out[1] = sabs;
                out[2] = ssq;
                out[3] = swsq;
            }
            cnt = sabs = ssq = swsq = 0.0;
        }
        __syncthreads();        // the LDS and the scratch slice are reused by the next unit of this workgroup
    }
}

}  // namespace

namespace fsnap {

// workgroups per CU that fit: 158 - 165 VGPRs allow three, the LDS (22 / 42 / 72 / 132 KB for nt <= 2 / 4 / 6 / 9) as many or fewer
int path_blocks_per_cu(int K) {
    const int nt = (K + 15) / 16;
    return nt <= 4 ? 3 : nt <= 6 ? 2 : 1;
}

hipError_t launch_ridge_path(int nblocks, const double* A, int64_t lda, int K, const double* wpack, const double* b,
                             const int* idx, const int64_t* off, int nunits, const double* G, const double* c,
                             const double* alphas, int Q, const unsigned char* rcls, int nclass, double* Bg, double* sums,
                             double* info, double* pred, int64_t m, hipStream_t st) {
    if (nunits <= 0 || nblocks <= 0) return hipSuccess;
    if (K < 1 || K > PATH_MAX_K) return hipErrorInvalidValue;
    const PathArgs a = {A, lda, K, wpack, b, idx, off, nunits, G, c, alphas, Q, rcls, nclass, Bg, sums, info, pred, m};
    const dim3 grid((unsigned)nblocks);
    const int nt = (K + 15) / 16;
    if (nt <= 2) fsnap_path_k<2><<<grid, 256, 0, st>>>(a);
    else if (nt <= 4) fsnap_path_k<4><<<grid, 256, 0, st>>>(a);
    else if (nt <= 6) fsnap_path_k<6><<<grid, 256, 0, st>>>(a);
    else fsnap_path_k<9><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace fsnap
