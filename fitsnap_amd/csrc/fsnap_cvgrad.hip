// fsnap_cvgrad.hip — gradient of the cross-validated cost of group-weight candidates over their scales
// (fsnap_cv_candidates_grad; the objective, omega and the descent are solvers/candidates_cv_grad.py).  gfx950 only.
//
// With the blocks B[f][c] and R[f][c] = T[c] - B[f][c] of fsnap_cv.hip, the refits beta[p][f] of kernel V1 and the host's
// per-category coefficients omega[p][c] of the objective, the adjoint of the K x K solve of problem (p, f) is
//     g   = 2 sum_c omega[p][c] (B[f][c].G beta - B[f][c].r)
//     lam = H^-1 g                        (H = sum_c S[p][c]^2 R[f][c].G + alpha I on the live columns: kernel V1's system)
//     D[p][f][c] = lam . (R[f][c].r - R[f][c].G beta)
// and dJ/dS[p][c] = 2 S[p][c] sum_f D[p][f][c], dJ/dlog alpha[p] = -alpha sum_f lam . beta (both sums on the host).
//   G1  fsnap_cvgrad_rhs_k       one workgroup per (row tile, 16-candidate tile, fold): it owns 16 rows of every block of the fold;
//                                each wave runs a quarter of the categories, c ascending; the block's rows are the A operand of
//                                v_mfma_f64_16x16x4_f64, omega[c][e] beta[k][e] the B operand (beta staged in LDS once, scaled per
//                                category), so one accumulator tile per wave holds sum_c B.G (omega beta) and four scalars beside
//                                it sum_c omega B.r; the waves' partials are added in index order.
//       fsnap_cvgrad_bilinear_k  one workgroup per (category, 16-candidate tile, fold): wave w takes the row tiles w, w + 4,
//                                w + 8 of R[f][c], forms R.G beta per tile on the matrix pipe and adds lam[row] (R.r[row] - y)
//                                per lane, rows ascending; the four k-slot lanes are summed by ks_sum, the waves in index order.
//   G2  fsnap_cvgrad_solve_k     kernel V1 of fsnap_cv.hip with g as the right-hand side (its own copy of that body: V1's code
//                                and with it V1's bits stay as they are).
// Both G1 kernels read a block once per 16 candidates.  fp64, no atomics; every sum runs in an order fixed by the problem alone
// (c ascending within a wave's quarter, the quarters in index order, k ascending in steps of 8, rows ascending; a candidate is one column of the MFMA tile and no lane of another
// column enters it): a candidate's bits do not depend on the batch, the grid or the run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fsnap_device_common.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

constexpr int CVG_THREADS = 256;
constexpr int CVG_WAVES = CVG_THREADS / 64;
constexpr int CVG_TAB = CV_MAX_K * 16;           // doubles of one staged table (K8 <= 144 rows of 16 candidates)

__device__ __forceinline__ int cvg_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// kernel V1's combination (c ascending, one fma per term, the loads of eight categories in flight)
template <int N>
__device__ __forceinline__ void cvg_combine(const double* __restrict__ Sp, int C, const double* __restrict__ base, int64_t T,
                                            const int64_t (&at)[N], double (&v)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = 0.0;
    int c = 0;
    for (; c + 8 <= C; c += 8) {
        double r[N][8], s2[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double sv = Sp[c + u];
            s2[u] = sv * sv;
#pragma unroll
            for (int n = 0; n < N; ++n) r[n][u] = base[(int64_t)(c + u) * T + at[n]];
        }
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int u = 0; u < 8; ++u) v[n] = __builtin_fma(s2[u], r[n][u], v[n]);
    }
    for (; c < C; ++c) {
        const double sv = Sp[c];
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] = __builtin_fma(sv * sv, base[(int64_t)c * T + at[n]], v[n]);
    }
}

// y[row ks + 4 g of the tile][candidate e] += sum_k G[row][k] sc tab[k][e] for the 16 rows `row0 ...` of the K x K square G:
// lane (e, ks) holds G[row0 + e][k0 + 2 ks + {0, 1}] and the matching table slots, two MFMAs per 8 columns, k0 ascending.  Rows
// and columns past K are zeros (the table is zero-padded to K8 rows).
template <bool SCALED>
__device__ __forceinline__ d4 cvg_tile(const double* __restrict__ G, int K, int K8, int row0, const double* tab, int e, int ks,
                                       double sc, d4 y) {
    const int row = row0 + e;
    const bool valid = row < K;
    const double* src = G + (int64_t)(valid ? row : 0) * K;
    for (int k0 = 0; k0 < K8; k0 += 8) {
        const int ka = k0 + 2 * ks;
        double a0 = 0.0, a1 = 0.0;
        if (valid && ka < K) a0 = src[ka];
        if (valid && ka + 1 < K) a1 = src[ka + 1];
        double b0 = tab[ka * 16 + e], b1 = tab[(ka + 1) * 16 + e];
        if (SCALED) {
            b0 *= sc;
            b1 *= sc;
        }
        y = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, y, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, y, 0, 0, 0);
    }
    return y;
}

// Kernel G1, RHS epilogue.  grid (NT, tiles, F), NT = ceil(K / 16): a workgroup owns 16 rows of every block of the fold; wave w takes
// the categories [w Cq, (w + 1) Cq), Cq = ceil(C / 4), in ascending order, and the four waves' partial tiles are added in index
// order through LDS -- an order fixed by C alone.
__global__ __launch_bounds__(CVG_THREADS) void fsnap_cvgrad_rhs_k(const double* __restrict__ stats, const double* __restrict__ betaT,
                                                                  const double* __restrict__ omegaT, int P, int F, int C, int K,
                                                                  double* __restrict__ g) {
    __shared__ double bt[CVG_TAB];
    __shared__ double red[CVG_WAVES * 8 * 64];
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, ks = lane >> 4, wave = tid >> 6;
    const int f = blockIdx.z, tile = blockIdx.y;
    const int K8 = (K + 7) / 8 * 8, KK = K * K;
    const int64_t T = (int64_t)KK + K + 3;
    const double* src = betaT + ((int64_t)tile * F + f) * K8 * 16;
    for (int i = tid; i < K8 * 16; i += CVG_THREADS) bt[i] = src[i];
    __syncthreads();
    const int row0 = blockIdx.x * 16;            // < K by the grid
    const double* om = omegaT + (int64_t)tile * C * 16;
    const int Cq = (C + CVG_WAVES - 1) / CVG_WAVES;
    const int c1 = (wave + 1) * Cq < C ? (wave + 1) * Cq : C;
    d4 y = {0.0, 0.0, 0.0, 0.0};
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = wave * Cq; c < c1; ++c) {
        const double w = om[c * 16 + e];
        const double* blk = stats + ((int64_t)f * C + c) * T;
        y = cvg_tile<true>(blk, K, K8, row0, bt, e, ks, w, y);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = row0 + ks + 4 * q;
            const double rv = row < K ? blk[KK + row] : 0.0;
            r[q] = __builtin_fma(w, rv, r[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        red[(wave * 8 + q) * 64 + lane] = y[q];
        red[(wave * 8 + 4 + q) * 64 + lane] = r[q];
    }
    __syncthreads();
    const int p = tile * 16 + e;
    if (wave != 0 || p >= P) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double ys = red[q * 64 + lane], rs = red[(4 + q) * 64 + lane];
#pragma unroll
        for (int w = 1; w < CVG_WAVES; ++w) {
            ys += red[(w * 8 + q) * 64 + lane];
            rs += red[(w * 8 + 4 + q) * 64 + lane];
        }
        const int row = row0 + ks + 4 * q;
        if (row < K) g[((int64_t)p * F + f) * K + row] = 2.0 * (ys - rs);
    }
}

// Kernel G1, bilinear epilogue.  grid (C, tiles, F); D[((tile F + f) C + c) 16 + e].
__global__ __launch_bounds__(CVG_THREADS) void fsnap_cvgrad_bilinear_k(const double* __restrict__ rest, const double* __restrict__ betaT,
                                                                       const double* __restrict__ lamT, int F, int C, int K,
                                                                       double* __restrict__ D) {
    __shared__ double bt[CVG_TAB];
    __shared__ double lt[CVG_TAB];
    __shared__ double red[CVG_WAVES * 16];
    const int tid = threadIdx.x, lane = tid & 63, e = lane & 15, ks = lane >> 4, wave = tid >> 6;
    const int c = blockIdx.x, tile = blockIdx.y, f = blockIdx.z;
    const int K8 = (K + 7) / 8 * 8, KK = K * K;
    const int64_t T = (int64_t)KK + K + 3;
    const int64_t tab = ((int64_t)tile * F + f) * K8 * 16;
    for (int i = tid; i < K8 * 16; i += CVG_THREADS) {
        bt[i] = betaT[tab + i];
        lt[i] = lamT[tab + i];
    }
    __syncthreads();
    const double* blk = rest + ((int64_t)f * C + c) * T;
    double s = 0.0;
    for (int row0 = wave * 16; row0 < K; row0 += CVG_WAVES * 16) {
        d4 y = {0.0, 0.0, 0.0, 0.0};
        y = cvg_tile<false>(blk, K, K8, row0, bt, e, ks, 1.0, y);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = row0 + ks + 4 * q;
            if (row < K) {
                const double res = blk[KK + row] - y[q];
                s = __builtin_fma(lt[row * 16 + e], res, s);
            }
        }
    }
    s = ks_sum(s);
    if (ks == 0) red[wave * 16 + e] = s;
    __syncthreads();
    if (tid < 16) {
        double v = red[tid];
#pragma unroll
        for (int w = 1; w < CVG_WAVES; ++w) v += red[w * 16 + tid];
        D[(((int64_t)tile * F + f) * C + c) * 16 + tid] = v;
    }
}

// Kernel G2: fsnap_cv_solve_k with g[prob][K] as the right-hand side -- the same combination over c, live rule, Jacobi scaling,
// right-looking Cholesky, substitutions and pivot tolerance.  lam[prob][K] (0 on dead columns, NaN with status 1) and the same
// values into lamT[p / 16][f][k][p % 16] (zeroed by the caller); info[prob][2] = status, smallest scaled pivot met.
__global__ __launch_bounds__(CVG_THREADS) void fsnap_cvgrad_solve_k(const double* __restrict__ rest, const double* __restrict__ total,
                                                                    const double* __restrict__ S, const double* __restrict__ g, int P,
                                                                    int F, int C, int K, double alpha, double pivot_tol,
                                                                    double* __restrict__ lam_out, double* __restrict__ lamT,
                                                                    double* __restrict__ info_out) {
    extern __shared__ __attribute__((aligned(16))) double cvg_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t T = (int64_t)K * K + K + 3;
    const int K8 = (K + 7) / 8 * 8;
    double* tri = cvg_lds;                       // the layout of kernel V1 (cv_lds_bytes)
    double* dsc = tri + K * (K + 1) / 2;
    double* rhs = dsc + K;
    double* yv = rhs + K;
    double* cv0 = yv + K;
    double* dl = cv0 + K;
    double* coef = dl + K;
    int* idx = (int*)(coef + K);
    int* flag = idx + K;
    int* cnt = flag + K;
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const int nprob = P * F;
    for (int prob = blockIdx.x; prob < nprob; prob += gridDim.x) {
        const int p = prob / F, f = prob - p * F;
        const double* Sp = S + (int64_t)p * C;
        const double* Rf = rest + (int64_t)f * C * T;
        if (tid < K) {
            const int64_t at[1] = {(int64_t)tid * K + tid};
            double tp[1], q[1];
            cvg_combine<1>(Sp, C, total, T, at, tp);
            cvg_combine<1>(Sp, C, Rf, T, at, q);
            const bool dead = tp[0] == 0.0 || q[0] <= pivot_tol * tp[0];
            dsc[tid] = dead ? 1.0 : sqrt(q[0] + alpha);
            flag[tid] = dead ? 0 : 1;
            coef[tid] = 0.0;
        }
        __syncthreads();
        if (wave == 0) {
            int base = 0;
            for (int j0 = 0; j0 < K; j0 += 64) {
                const int j = j0 + lane;
                const bool on = j < K && flag[j] != 0;
                const unsigned long long mask = __ballot(on);
                if (on) idx[base + __popcll(mask & ((1ull << lane) - 1ull))] = j;
                base += __popcll(mask);
            }
            if (lane == 0) cnt[0] = base;
        }
        __syncthreads();
        const int k = cnt[0];
        for (int a = wave; a < k; a += CVG_WAVES) {
            const int ia = idx[a];
            const double da = dsc[ia];
            if (lane > a) continue;
            int64_t at[3];
            double v[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int b = lane + 64 * n;
                at[n] = (int64_t)ia * K + idx[b <= a ? b : lane];
            }
            cvg_combine<3>(Sp, C, Rf, T, at, v);
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int b = lane + 64 * n;
                if (b > a) break;
                double h = v[n];
                if (b == a) h += alpha;
                tri[cvg_tri(a, b)] = h / (da * dsc[idx[b]]);
            }
        }
        if (tid < k) {
            const int ia = idx[tid];
            rhs[tid] = g[(int64_t)prob * K + ia] / dsc[ia];
        }
        __syncthreads();
        double minpiv = inf;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
            const double piv = tri[cvg_tri(j, j)];
            minpiv = piv < minpiv ? piv : minpiv;
            if (!(piv > pivot_tol)) {
                if (piv != piv) minpiv = piv;
                ok = false;
                break;
            }
            const double ljj = sqrt(piv);
            const double yj = rhs[j] / ljj;
            for (int i = j + 1 + tid; i < k; i += CVG_THREADS) {
                const double v = tri[cvg_tri(i, j)] / ljj;
                tri[cvg_tri(i, j)] = v;
                cv0[i] = v;
                rhs[i] = __builtin_fma(-v, yj, rhs[i]);
            }
            if (tid == 0) {
                dl[j] = ljj;
                yv[j] = yj;
            }
            __syncthreads();
            for (int i = j + 1 + wave; i < k; i += CVG_WAVES) {
                const double li = cv0[i];
                double* row = tri + cvg_tri(i, 0);
                for (int c = j + 1 + lane; c <= i; c += 64) row[c] = __builtin_fma(-li, cv0[c], row[c]);
            }
            __syncthreads();
        }
        if (ok) {
            for (int i = k - 1; i >= 0; --i) {
                const double xi = yv[i] / dl[i];
                const double* row = tri + cvg_tri(i, 0);
                for (int j = tid; j < i; j += CVG_THREADS) yv[j] = __builtin_fma(-row[j], xi, yv[j]);
                if (tid == 0) cv0[i] = xi;
                __syncthreads();
            }
            if (tid < k) {
                const int ia = idx[tid];
                coef[ia] = cv0[tid] / dsc[ia];
            }
        }
        __syncthreads();
        if (tid < K) {
            const double v = ok ? coef[tid] : nan;
            lam_out[(int64_t)prob * K + tid] = v;
            lamT[(((int64_t)(p >> 4) * F + f) * K8 + tid) * 16 + (p & 15)] = v;
        }
        if (tid == 0) {
            double* io = info_out + (int64_t)prob * 2;
            io[0] = ok ? 0.0 : 1.0;
            io[1] = minpiv;
        }
        __syncthreads();                         // the next problem refills the vectors
    }
}

}  // namespace

hipError_t launch_cvgrad_rhs(const double* stats, const double* betaT, const double* omegaT, int P, int F, int C, int K, double* g,
                             hipStream_t st) {
    if (K < 1 || K > CV_MAX_K || P < 1 || F < 1 || C < 1) return hipErrorInvalidValue;
    const int NT = (K + 15) / 16, tiles = (P + 15) / 16;
    if (tiles > 65535 || F > 65535) return hipErrorInvalidValue;
    fsnap_cvgrad_rhs_k<<<dim3((unsigned)NT, (unsigned)tiles, (unsigned)F), CVG_THREADS, 0, st>>>(
        stats, betaT, omegaT, P, F, C, K, g);
    return hipGetLastError();
}

hipError_t launch_cvgrad_solve(int nblocks, const double* rest, const double* total, const double* S, const double* g, int P, int F,
                               int C, int K, double alpha, double* lam, double* lamT, double* info, hipStream_t st) {
    if (K < 1 || K > CV_MAX_K || nblocks < 1) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_cvgrad_solve_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)cv_lds_bytes(CV_MAX_K));
    if (e != hipSuccess) return e;
    fsnap_cvgrad_solve_k<<<dim3((unsigned)nblocks), dim3(CVG_THREADS), cv_lds_bytes(K), st>>>(rest, total, S, g, P, F, C, K, alpha,
                                                                                              LOCO_PIVOT_TOL, lam, lamT, info);
    return hipGetLastError();
}

hipError_t launch_cvgrad_bilinear(const double* rest, const double* betaT, const double* lamT, int P, int F, int C, int K, double* D,
                                  hipStream_t st) {
    if (K < 1 || K > CV_MAX_K || P < 1 || F < 1 || C < 1) return hipErrorInvalidValue;
    const int tiles = (P + 15) / 16;
    if (tiles > 65535 || F > 65535 || (int64_t)C * tiles * F > ((int64_t)1 << 24) - 1) return hipErrorInvalidValue;
    fsnap_cvgrad_bilinear_k<<<dim3((unsigned)C, (unsigned)tiles, (unsigned)F), CVG_THREADS, 0, st>>>(rest, betaT, lamT, F, C, K, D);
    return hipGetLastError();
}

}  // namespace fsnap
