// fsnap_ard.hip — grouped K-fold ARD threshold paths on the per-fold statistics (fsnap_ard_path; the grid, the hyper-parameters,
// the host route and the picks are solvers/ard_path.py).  ARD's iteration (ARD._ard_loop, scikit-learn's ARDRegression.fit)
// touches the rows only through (X^T X, X^T y, |y|^2, n), so with one packed block [G_f | c_f | bb_f, sum wb, n_f] per fold
// (fsnap_cat_normal_eq; summed by kernel S1 of fsnap_lasso.hip) the training system of fold f is "total minus block f" and the
// (F + 1) x Q problems (fold f left out, or none; setting q) are independent, strictly sequential iterations on K x K systems.
//   Kernel A1: one workgroup of 256 threads (four waves, one per SIMD) per problem, grid-stride.  The working matrix of the
//              KEPT columns, W = diag(lambda / d^2) + alpha Qm / (d d^T), sits in LDS as the packed lower triangle (K = 144:
//              83 520 B + 10 K-vectors; two triangles would not fit, so W is gathered again from the fold blocks in global
//              memory -- L2-resident -- every iteration).  Per iteration: gather, Cholesky W = L L^T (right-looking, the scaled
//              column copied to a contiguous vector so that the trailing update reads rows and that vector only), M = L^-1 in
//              place (column by column from the last, one wave per row, the column double-buffered: one barrier per column),
//              z = M qs by rows, then per column a: diag Sigma_a = sum_i M_ia^2 and cs_a = sum_i M_ia z_i (lane a walks down
//              column a: consecutive lanes, consecutive addresses), coef = alpha cs / d, the three sums of the residual and
//              sum gamma, the lambda / alpha / keep updates and an ORDERED compaction of the kept columns (ballot prefix).
//              LDS accesses: rows of the packed triangle are contiguous (conflict-free); the two column walks of a
//              factorisation step (scaling column j, copying it for the inverse) touch k - j addresses with a growing stride
//              once per column and are left as they are.  Barriers: 2 per column in the factorisation, 1 in the inverse.
// fp64 VALU only, no atomics.  Every sum runs in an order fixed by the problem alone (lane l adds the elements l, l + 64,
// l + 128 in that order, then the xor butterfly of fsnap_wave_sum.h; column walks run top to bottom): a problem's result is
// bit-identical run to run and under any permutation or subset of the grid.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fsnap_fold_body.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

constexpr int ARD_THREADS = 256;
constexpr int ARD_WAVES = ARD_THREADS / 64;

__device__ __forceinline__ int tri_at(int i, int j) { return i * (i + 1) / 2 + j; }

// sum of term(e) over e in [0, n), n <= 192: lane l adds e = l, l + 64, l + 128, then the butterfly; every wave that calls it
// gets the same bits in every lane
template <class Term>
__device__ __forceinline__ double sum_by_wave(int n, int lane, Term&& term) {
    double s = 0.0;
    for (int e = lane; e < n; e += 64) s += term(e);
    return wave_sum(s);
}

// The K-vectors and the state of one problem in LDS.
struct ArdLds {
    double* tri;      // packed lower triangle of the kept system: W, then L (diagonal apart, in dl), then M = L^-1
    double* lam;      // lambda by column
    double* dsc;      // d by column (1 for dead columns)
    double* coef;     // coefficients by column (0 outside the kept set)
    double* cold;     // the coefficients of the previous iteration
    double* qvk;      // qv of the kept columns, by position
    double* qs;       // qv / d of the kept columns, by position
    double* dl;       // diagonal of L by position
    double* cv0;      // work column (double-buffered with cv1), gamma by position
    double* cv1;
    double* rv;       // row results by position (z, Qm coef)
    int* idx;         // the kept columns in ascending order
    int* flag;        // keep flag by column
    int* cnt;         // number of kept columns
};

// Gathers W of the kept set, factors and inverts it, and leaves in every thread a < k: cs = (W^-1 qs)_a and sig = (W^-1)_aa.
// Returns false (in every thread) at a pivot that is not positive; the smallest pivot met goes into minpiv.
__device__ bool ard_solve_kept(const ArdLds& s, const double* __restrict__ total, const double* __restrict__ Gf, int K, int k,
                               double alpha, double& minpiv, double& cs, double& sig) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KK = K * K;
    // gather and scale: W_ab = alpha Qm_ab / (d_a d_b), + lambda_a / d_a^2 on the diagonal
    for (int a = wave; a < k; a += ARD_WAVES) {
        const int ia = s.idx[a];
        const double da = s.dsc[ia];
        for (int b = lane; b <= a; b += 64) {
            const int ib = s.idx[b];
            const int64_t at = (int64_t)ia * K + ib;                  // ia >= ib: the lower triangle of the blocks
            double v = total[at];
            if (Gf) v -= Gf[at];
            v = alpha * (v / (da * s.dsc[ib]));
            if (b == a) v = s.lam[ia] / (da * da) + v;
            s.tri[tri_at(a, b)] = v;
        }
    }
    if (tid < k) {
        const int ia = s.idx[tid];
        double v = total[KK + ia];
        if (Gf) v -= Gf[KK + ia];
        s.qvk[tid] = v;
        s.qs[tid] = v / s.dsc[ia];
    }
    __syncthreads();
    // Cholesky, right-looking
    for (int j = 0; j < k; ++j) {
        const double piv = s.tri[tri_at(j, j)];
        minpiv = fmin(minpiv, piv);
        if (!(piv > 0.0)) return false;                               // uniform: every thread read the same value
        const double ljj = sqrt(piv);
        for (int i = j + 1 + tid; i < k; i += ARD_THREADS) {
            const double v = s.tri[tri_at(i, j)] / ljj;
            s.tri[tri_at(i, j)] = v;
            s.cv0[i] = v;
        }
        if (tid == 0) s.dl[j] = ljj;
        __syncthreads();
        for (int i = j + 1 + wave; i < k; i += ARD_WAVES) {
            const double li = s.cv0[i];
            double* row = s.tri + tri_at(i, 0);
            for (int c = j + 1 + lane; c <= i; c += 64) row[c] -= li * s.cv0[c];
        }
        __syncthreads();
    }
    // M = L^-1 in place, from the last column: M_jj = 1 / L_jj, M_ij = -(sum_{c = j + 1 .. i} M_ic L_cj) M_jj
    for (int j = k - 1; j >= 0; --j) {
        double* x = (j & 1) ? s.cv1 : s.cv0;
        for (int i = j + 1 + tid; i < k; i += ARD_THREADS) x[i] = s.tri[tri_at(i, j)];
        const double mjj = 1.0 / s.dl[j];
        __syncthreads();
        for (int i = j + 1 + wave; i < k; i += ARD_WAVES) {
            const double* row = s.tri + tri_at(i, 0);
            double acc = 0.0;
            for (int c = j + 1 + lane; c <= i; c += 64) acc += row[c] * x[c];
            acc = wave_sum(acc);
            if (lane == 0) s.tri[tri_at(i, j)] = -acc * mjj;
        }
        if (tid == 0) s.tri[tri_at(j, j)] = mjj;
        // no barrier here: the next column fills the other work vector and touches column j - 1 of the triangle, which this
        // step neither reads nor writes
    }
    __syncthreads();
    // z = M qs by rows
    for (int i = wave; i < k; i += ARD_WAVES) {
        const double* row = s.tri + tri_at(i, 0);
        double acc = 0.0;
        for (int c = lane; c <= i; c += 64) acc += row[c] * s.qs[c];
        acc = wave_sum(acc);
        if (lane == 0) s.rv[i] = acc;
    }
    __syncthreads();
    // column a of M, top to bottom: cs_a = sum_i M_ia z_i, sig_a = sum_i M_ia^2
    cs = 0.0;
    sig = 0.0;
    if (tid < k) {
        for (int i = tid; i < k; ++i) {
            const double m = s.tri[tri_at(i, tid)];
            cs += m * s.rv[i];
            sig += m * m;
        }
    }
    __syncthreads();                                                  // rv is free again
    return true;
}

// Kernel A1.  hyper[p][6] = alpha_1, alpha_2, lambda_1, lambda_2, threshold_lambda, alpha_init.
__global__ __launch_bounds__(ARD_THREADS) void fsnap_ard_path_k(const double* __restrict__ folds, const double* __restrict__ total,
                                                                const double* __restrict__ hyper, int K, int F, int Q,
                                                                int max_iter, double tol, double pivot_tol,
                                                                double* __restrict__ coef_out, double* __restrict__ lambda_out,
                                                                double* __restrict__ info_out, double* __restrict__ heldout) {
    extern __shared__ __attribute__((aligned(16))) double ard_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KK = K * K;
    ArdLds s;
    s.tri = ard_lds;
    s.lam = s.tri + K * (K + 1) / 2;
    s.dsc = s.lam + K;
    s.coef = s.dsc + K;
    s.cold = s.coef + K;
    s.qvk = s.cold + K;
    s.qs = s.qvk + K;
    s.dl = s.qs + K;
    s.cv0 = s.dl + K;
    s.cv1 = s.cv0 + K;
    s.rv = s.cv1 + K;
    s.idx = (int*)(s.rv + K);
    s.flag = s.idx + K;
    s.cnt = s.flag + K;
    const int nprob = (F + 1) * Q;
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);

    // the kept columns in ascending order from the flags (wave 0; a ballot prefix, not arrival order)
    auto compact = [&]() {
        if (wave == 0) {
            int base = 0;
            for (int j0 = 0; j0 < K; j0 += 64) {
                const int j = j0 + lane;
                const bool on = j < K && s.flag[j] != 0;
                const unsigned long long mask = __ballot(on);
                if (on) s.idx[base + __popcll(mask & ((1ull << lane) - 1ull))] = j;
                base += __popcll(mask);
            }
            if (lane == 0) s.cnt[0] = base;
        }
    };

    for (int p = blockIdx.x; p < nprob; p += gridDim.x) {
        const int f = p / Q;
        const FoldView fv = fold_view(folds, total, f, F, K);
        const double* Gf = fv.Gf;
        const double y2 = fv.y2, n = fv.n;
        const double* hy = hyper + (int64_t)p * 6;
        const double alpha_1 = hy[0], alpha_2 = hy[1], lambda_1 = hy[2], lambda_2 = hy[3], thr = hy[4];
        double alpha = hy[5];
        if (tid < K) {
            const int64_t at = (int64_t)tid * K + tid;
            const double tjj = total[at];
            const double qjj = Gf ? tjj - Gf[at] : tjj;
            const bool dead = fold_dead(tjj, qjj, pivot_tol);
            s.dsc[tid] = dead ? 1.0 : sqrt(qjj);
            s.lam[tid] = 1.0;
            s.coef[tid] = 0.0;
            s.cold[tid] = 0.0;
            s.flag[tid] = dead ? 0 : 1;
        }
        __syncthreads();
        compact();
        __syncthreads();
        int k = s.cnt[0];
        int status = k > 0 ? 2 : 0, iters = 0;
        double minpiv = inf, delta = inf, cs, sig;
        for (int it = 0; it < max_iter && k > 0; ++it) {
            iters = it + 1;
            if (!ard_solve_kept(s, total, Gf, K, k, alpha, minpiv, cs, sig)) {
                status = 1;
                break;
            }
            int ia = 0;
            double ca = 0.0, gamma = 0.0;
            if (tid < k) {
                ia = s.idx[tid];
                const double da = s.dsc[ia];
                ca = alpha * (cs / da);
                gamma = 1.0 - s.lam[ia] * (sig / (da * da));
                s.coef[ia] = ca;
                s.cv0[tid] = gamma;
                s.cv1[tid] = ca;
            }
            __syncthreads();
            // Qm coef over the kept columns, one wave per row
            for (int a = wave; a < k; a += ARD_WAVES) {
                const int ra = s.idx[a];
                double acc = 0.0;
                for (int b = lane; b < k; b += 64) {
                    const int rb = s.idx[b];
                    const int64_t at = ra >= rb ? (int64_t)ra * K + rb : (int64_t)rb * K + ra;
                    double v = total[at];
                    if (Gf) v -= Gf[at];
                    acc += v * s.cv1[b];
                }
                acc = wave_sum(acc);
                if (lane == 0) s.rv[a] = acc;
            }
            __syncthreads();
            // every wave forms the same three sums: identical bits in every thread
            const double cq = sum_by_wave(k, lane, [&](int e) { return s.cv1[e] * s.qvk[e]; });
            const double cQc = sum_by_wave(k, lane, [&](int e) { return s.cv1[e] * s.rv[e]; });
            const double gsum = sum_by_wave(k, lane, [&](int e) { return s.cv0[e]; });
            const double sse = fmax(y2 - 2.0 * cq + cQc, 0.0);
            bool bad = false;
            if (tid < k) {
                const double l = (gamma + 2.0 * lambda_1) / (ca * ca + 2.0 * lambda_2);
                bad = !isfinite(l);
                s.lam[ia] = l;
                const bool on = l < thr;
                s.flag[ia] = on ? 1 : 0;
                if (!on) s.coef[ia] = 0.0;
            }
            alpha = (n - gsum + 2.0 * alpha_1) / (sse + 2.0 * alpha_2);
            bad = bad || !isfinite(alpha);
            if (__syncthreads_or(bad ? 1 : 0)) {
                status = 1;
                break;
            }
            delta = sum_by_wave(K, lane, [&](int e) { return fabs(s.cold[e] - s.coef[e]); });
            compact();
            __syncthreads();
            if (tid < K) s.cold[tid] = s.coef[tid];
            k = s.cnt[0];
            __syncthreads();
            if ((it > 0 && delta < tol) || k == 0) {
                status = 0;
                break;
            }
        }
        if (status != 1 && k > 0) {
            // the final coefficients of the kept set under the last lambda and alpha
            if (ard_solve_kept(s, total, Gf, K, k, alpha, minpiv, cs, sig)) {
                if (tid < k) {
                    const int ia = s.idx[tid];
                    s.coef[ia] = alpha * (cs / s.dsc[ia]);
                }
            } else {
                status = 1;
            }
        }
        __syncthreads();
        if (tid < K) {
            if (status == 1) {
                s.coef[tid] = nan;
                s.lam[tid] = nan;
            }
            coef_out[(int64_t)p * K + tid] = s.coef[tid];
            lambda_out[(int64_t)p * K + tid] = s.lam[tid];
        }
        if (tid == 0) {
            double* io = info_out + (int64_t)p * 6;
            io[0] = (double)iters;
            io[1] = status == 1 ? 0.0 : (double)k;
            io[2] = alpha;
            io[3] = delta;
            io[4] = minpiv;
            io[5] = (double)status;
        }
        __syncthreads();
        if (Gf) {
            // weighted squared error of fold f under its own refit, from the fold's statistics: bb_f - 2 beta . c_f + beta^T G_f beta
            for (int i = wave; i < K; i += ARD_WAVES) {
                const double* row = Gf + (int64_t)i * K;
                double acc = 0.0;
                for (int j = lane; j < K; j += 64) acc += row[j] * s.coef[j];
                acc = wave_sum(acc);
                if (lane == 0) s.rv[i] = acc;
            }
            __syncthreads();
            if (wave == 0) {
                const double s1 = sum_by_wave(K, lane, [&](int e) { return s.coef[e] * Gf[KK + e]; });
                const double s2 = sum_by_wave(K, lane, [&](int e) { return s.coef[e] * s.rv[e]; });
                // p = f Q + q for f < F
                if (lane == 0) fold_heldout_store(heldout + (int64_t)p * 3, fv.n_f, fv.bb_f - 2.0 * s1 + s2, fv.bb_f);
            }
        }
        __syncthreads();                                              // the next problem refills the vectors
    }
}

}  // namespace

size_t ard_lds_bytes(int K) { return ((size_t)K * (K + 1) / 2 + 10 * (size_t)K) * 8 + (2 * (size_t)K + 2) * 4; }

int ard_blocks_per_cu(int K) {
    const size_t per = (size_t)160 * 1024 / (ard_lds_bytes(K) + 512);
    return per < 1 ? 1 : per > 4 ? 4 : (int)per;
}

hipError_t launch_ard_path(int nblocks, const double* folds, const double* total, const double* hyper, int K, int F, int Q,
                           int max_iter, double tol, double* coef, double* lambda, double* info, double* heldout, hipStream_t st) {
    if (K < 1 || K > ARD_MAX_K || nblocks < 1) return hipErrorInvalidValue;
    // set on every launch: the attribute belongs to the current device, and the call costs microseconds next to the kernel
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_ard_path_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)ard_lds_bytes(ARD_MAX_K));
    if (e != hipSuccess) return e;
    fsnap_ard_path_k<<<dim3((unsigned)nblocks), dim3(ARD_THREADS), ard_lds_bytes(K), st>>>(
        folds, total, hyper, K, F, Q, max_iter, tol, LOCO_PIVOT_TOL, coef, lambda, info, heldout);
    return hipGetLastError();
}

}  // namespace fsnap
