// fsnap_lasso.hip — grouped K-fold LASSO alpha paths on the per-fold statistics (fsnap_lasso_path; the host algebra and the
// tables are solvers/lasso_path.py).  Coordinate descent touches the rows only through (X^T X, X^T y, |y|^2), so with one packed
// block [G_f | c_f | bb_f, sum wb, n_f] per fold (fsnap_cat_normal_eq) the training system of fold f is "total minus block f"
// and the (F + 1) x Q problems (fold f left out, or none; alpha_q) are independent K x K recurrences.
//   Kernel S1: fold blocks (the sum of nsub sub-blocks each, in index order) and the total T (the folds in index order); the
//              ARD and OMP paths (fsnap_ard.hip, fsnap_omp.hip) start from it too.
//   Kernel S2: one wave per problem, grid-stride.  The downdated matrix sits in LDS as the packed lower triangle (K = 144:
//              83 520 B; the square would not fit), H = Qm w and w in registers (lane l owns columns l, l + 64, l + 128), row
//              i + 1 is fetched from LDS while coordinate i is updated (the row does not depend on w).  The iteration is
//              fsnap_lasso_gram's statement for statement (fsnap_solve.cpp); only the three sums and the maximum of the duality
//              gap run as wave butterflies instead of left to right.  fp64 VALU only, no atomics, no barrier in the sweeps.
// A problem's result depends on its own (fold, alpha) only: bit-identical run to run and under any permutation of the grid.
#include <hip/hip_runtime.h>

#include "fsnap_fold_body.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

// Kernel S1.  grid ceil(T / 256); folds may be nullptr (nsub = 1: the blocks are the folds)
__global__ __launch_bounds__(256) void fsnap_fold_sums_k(const double* __restrict__ stats, int F, int nsub, int64_t T,
                                                         double* __restrict__ folds, double* __restrict__ total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T) return;
    double tot = 0.0;
    for (int f = 0; f < F; ++f) {
        const double* src = stats + (int64_t)f * nsub * T + e;
        double s = src[0];
        for (int k = 1; k < nsub; ++k) s += src[(int64_t)k * T];
        if (folds) folds[(int64_t)f * T + e] = s;
        tot = f == 0 ? s : tot + s;
    }
    total[e] = tot;
}

// Kernel S2.  NE = ceil(K / 64) columns per lane.  LDS: K (K + 1) / 2 + 2 K doubles (triangle, qv, beta).
template <int NE>
__global__ __launch_bounds__(64) void fsnap_lasso_cd_k(const double* __restrict__ folds, const double* __restrict__ total,
                                                       const double* __restrict__ alphas, int K, int F, int Q, int max_iter,
                                                       double tol, double pivot_tol, double* __restrict__ coef,
                                                       double* __restrict__ info, double* __restrict__ heldout) {
    extern __shared__ __attribute__((aligned(16))) double lasso_lds[];
    const int lane = threadIdx.x;
    const int KK = K * K;
    double* tri = lasso_lds;
    double* sq = tri + K * (K + 1) / 2;
    double* sw = sq + K;
    const int nprob = (F + 1) * Q;
    int col[NE];
    bool valid[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        col[e] = lane + 64 * e;
        valid[e] = col[e] < K;
    }
    for (int p = blockIdx.x; p < nprob; p += gridDim.x) {
        const int f = p / Q, q = p - f * Q;
        const FoldView fv = fold_view(folds, total, f, F, K);
        const double* Gf = fv.Gf;
        // the downdated lower triangle, subtracted while filling
#pragma unroll 4
        for (int x = lane; x < KK; x += 64) {
            const int i = x / K, j = x - i * K;
            if (j <= i) {
                double v = total[x];
                if (Gf) v -= Gf[x];
                tri[i * (i + 1) / 2 + j] = v;
            }
        }
        const double y2 = fv.y2, n = fv.n;
        const double l1 = alphas[q] * n;
        __syncthreads();
        unsigned long long dead[NE];
        double qv[NE], h[NE], w[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int j = valid[e] ? col[e] : 0;
            const double tjj = total[(int64_t)j * K + j];
            const double qjj = tri[j * (j + 1) / 2 + j];
            const bool d = valid[e] && fold_dead(tjj, qjj, pivot_tol);
            dead[e] = __ballot(d);
            double v = 0.0;
            if (valid[e] && !d) v = Gf ? total[KK + j] - Gf[KK + j] : total[KK + j];
            qv[e] = v;
            if (valid[e]) sq[j] = v;
            h[e] = 0.0;
            w[e] = 0.0;
        }
        __syncthreads();
        auto fetch = [&](int i, double(&r)[NE], double& qii, double& qi) {
            const int bi = i * (i + 1) / 2;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int j = col[e];
                const int at = valid[e] ? (j <= i ? bi + j : j * (j + 1) / 2 + i) : 0;
                const double v = tri[at];
                r[e] = valid[e] ? v : 0.0;
            }
            qii = tri[bi + i];
            qi = sq[i];
        };
        // no live coordinate (an empty training set, for one): the first sweep already is the fixed point
        bool any_live = false;
#pragma unroll
        for (int e = 0; e < NE; ++e) any_live = any_live || (__ballot(valid[e]) & ~dead[e]) != 0ull;
        const double gap_tol = tol * y2;
        double gap = gap_tol + 1.0;
        double nxt[NE], nqii, nqi;
        fetch(0, nxt, nqii, nqi);
        int it = 0;
        for (; it < max_iter; ++it) {
            double w_max = 0.0, d_w_max = 0.0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int iend = K < 64 * e + 64 ? K : 64 * e + 64;
                for (int i = 64 * e; i < iend; ++i) {
                    const int il = i & 63;
                    double cur[NE];
#pragma unroll
                    for (int g = 0; g < NE; ++g) cur[g] = nxt[g];
                    const double qii = nqii, qi = nqi;
                    fetch(i + 1 < K ? i + 1 : 0, nxt, nqii, nqi);
                    if ((dead[e] >> il) & 1ull) continue;
                    const double w_old = lane_bcast(w[e], il);
                    double hi = lane_bcast(h[e], il);
                    if (w_old != 0.0) {
#pragma unroll
                        for (int g = 0; g < NE; ++g) h[g] = __builtin_fma(-w_old, cur[g], h[g]);
                        hi = __builtin_fma(-w_old, qii, hi);
                    }
                    const double t = qi - hi;
                    const double mag = fabs(t) - l1;
                    double w_new = 0.0;
                    if (mag > 0.0) w_new = copysign(mag, t) / qii;
                    if (lane == il) w[e] = w_new;
                    if (w_new != 0.0) {
#pragma unroll
                        for (int g = 0; g < NE; ++g) h[g] = __builtin_fma(w_new, cur[g], h[g]);
                    }
                    d_w_max = fmax(d_w_max, fabs(w_new - w_old));
                    w_max = fmax(w_max, fabs(w_new));
                }
            }
            if (w_max == 0.0 || d_w_max / w_max < tol || it == max_iter - 1) {
                double qdw = 0.0, whw = 0.0, l1n = 0.0, dual = 0.0;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    qdw = __builtin_fma(w[e], qv[e], qdw);
                    whw = __builtin_fma(w[e], h[e], whw);
                    l1n += fabs(w[e]);
                    const bool live = valid[e] && !((dead[e] >> lane) & 1ull);
                    dual = fmax(dual, live ? fabs(qv[e] - h[e]) : 0.0);
                }
                qdw = wave_sum(qdw);
                whw = wave_sum(whw);
                l1n = wave_sum(l1n);
                dual = wave_max(dual);
                const double r2 = y2 + whw - 2.0 * qdw;
                double c = 1.0;
                if (dual > l1) {
                    c = l1 / dual;
                    gap = 0.5 * (r2 + r2 * c * c);
                } else {
                    gap = r2;
                }
                gap += l1 * l1n - c * y2 + c * qdw;
                if (gap < gap_tol || !any_live) {
                    ++it;
                    break;
                }
            }
        }
        if (it > max_iter) it = max_iter;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            if (valid[e]) {
                coef[(int64_t)p * K + col[e]] = w[e];
                sw[col[e]] = w[e];
            }
        if (lane == 0) {
            info[(int64_t)p * 4 + 0] = (double)it;
            info[(int64_t)p * 4 + 1] = gap;
            info[(int64_t)p * 4 + 2] = l1;
            info[(int64_t)p * 4 + 3] = n;
        }
        __syncthreads();
        if (Gf) {
            // weighted squared error of fold f under its own refit, from the fold's statistics: bb_f - 2 beta . c_f + beta^T G_f beta
            double acc[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[e] = 0.0;
#pragma unroll 4
            for (int i = 0; i < K; ++i) {
                const double bi = sw[i];
                const double* row = Gf + (int64_t)i * K;
#pragma unroll
                for (int e = 0; e < NE; ++e) acc[e] = __builtin_fma(valid[e] ? row[col[e]] : 0.0, bi, acc[e]);
            }
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const double cf = valid[e] ? Gf[KK + col[e]] : 0.0;
                s1 = __builtin_fma(w[e], cf, s1);
                s2 = __builtin_fma(w[e], acc[e], s2);
            }
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            // p = f Q + q for f < F
            if (lane == 0) fold_heldout_store(heldout + (int64_t)p * 3, fv.n_f, fv.bb_f - 2.0 * s1 + s2, fv.bb_f);
        }
        __syncthreads();                                       // the next problem refills the triangle
    }
}

}  // namespace

size_t lasso_lds_bytes(int K) { return ((size_t)K * (K + 1) / 2 + 2 * (size_t)K) * 8; }

int lasso_blocks_per_cu(int K) {
    const size_t per = (size_t)160 * 1024 / (lasso_lds_bytes(K) + 512);
    return per < 1 ? 1 : per > 8 ? 8 : (int)per;
}

hipError_t launch_fold_sums(const double* stats, int F, int nsub, int K, double* folds, double* total, hipStream_t st) {
    const int64_t T = (int64_t)K * K + K + 3;
    fsnap_fold_sums_k<<<dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st>>>(stats, F, nsub, T, folds, total);
    return hipGetLastError();
}

template <int NE>
static hipError_t lasso_cd_launch(int nblocks, size_t lds, const double* folds, const double* total, const double* alphas, int K,
                                  int F, int Q, int max_iter, double tol, double* coef, double* info, double* heldout,
                                  hipStream_t st) {
    // set on every launch: the attribute belongs to the current device, and the call costs microseconds next to the kernel
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_lasso_cd_k<NE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lasso_lds_bytes(64 * NE < LASSO_MAX_K ? 64 * NE : LASSO_MAX_K));
    if (e != hipSuccess) return e;
    fsnap_lasso_cd_k<NE><<<dim3((unsigned)nblocks), dim3(64), lds, st>>>(folds, total, alphas, K, F, Q, max_iter, tol,
                                                                         LOCO_PIVOT_TOL, coef, info, heldout);
    return hipGetLastError();
}

hipError_t launch_lasso_cd(int nblocks, const double* folds, const double* total, const double* alphas, int K, int F, int Q,
                           int max_iter, double tol, double* coef, double* info, double* heldout, hipStream_t st) {
    if (K < 1 || K > LASSO_MAX_K || nblocks < 1) return hipErrorInvalidValue;
    const size_t lds = lasso_lds_bytes(K);
    switch ((K + 63) / 64) {
        case 1: return lasso_cd_launch<1>(nblocks, lds, folds, total, alphas, K, F, Q, max_iter, tol, coef, info, heldout, st);
        case 2: return lasso_cd_launch<2>(nblocks, lds, folds, total, alphas, K, F, Q, max_iter, tol, coef, info, heldout, st);
        default: return lasso_cd_launch<3>(nblocks, lds, folds, total, alphas, K, F, Q, max_iter, tol, coef, info, heldout, st);
    }
}

}  // namespace fsnap
