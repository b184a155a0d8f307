// fsnap_cv.hip — grouped K-fold cross-validation of group-weight candidates on the per-(fold, category) statistics
// (fsnap_cv_candidates, fsnap_cv_candidate_rows; the folds, routes and tables are solvers/candidates_cv.py).  gfx950 only.
//
// The context holds F * C packed blocks B[f][c] = [G | r | bb, sum wb, n] (fsnap_cat_normal_eq, composite category f * C + c).
// Candidate p scales category c by S[p, c]; its refit without fold f is the K x K system
//     Qm = sum_c S[p,c]^2 (T[c].G - B[f,c].G),  qv = sum_c S[p,c]^2 (T[c].r - B[f,c].r),  T[c] = sum_f B[f,c]
// and every row of fold f is then scored under that refit, which never saw its configuration.
//   V0  fsnap_cv_total_k   T[c] = sum_f B[f][c], elementwise, folds in index order, and R[f][c] = T[c] - B[f][c]
//   V1  fsnap_cv_solve_k   one workgroup of 256 threads (four waves) per problem (p, f), grid-stride.  The C blocks R[f][.] of a
//                          problem are combined straight from global memory (they are L2 / Infinity-Cache resident) into the
//                          packed lower triangle of the LIVE columns in LDS (K = 144: 83 520 B + 6 K-vectors), Jacobi-scaled,
//                          factored (right-looking Cholesky, the scaled column copied to a contiguous vector so that the
//                          trailing update reads rows and that vector only; the forward substitution rides along with the
//                          column step) and back-substituted by rows.  Barriers: 2 per column forward, 1 per column backward.
//   V2  fsnap_cv_rows_k    a workgroup takes one chunk of the layout (<= 1024 rows of ONE composite category, so one fold),
//                          reads fold = category / C and multiplies the chunk's rows with that fold's coefficient table
//                          (betaT[f][k][16], zero-padded like kernel C3's) on v_mfma_f64_16x16x4_f64; per-wave partials of
//                          sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2 in the layout of kernel C3, so kernel C3R (WHAT = 0) reduces
//                          them per (candidate, composite category) in chunk order.
// fp64, no atomics.  Every sum runs in an order fixed by the problem alone (c ascending with one fma per term; lane l of a
// wave owns columns l, l + 64, l + 128 of a row; rows are dealt to waves by index): a problem's bits do not depend on the batch,
// the grid or the run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fsnap_device_common.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_WAVES = CV_THREADS / 64;

__device__ __forceinline__ int cv_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// v[n] = sum_c S[c]^2 base[c * T + at[n]], c ascending with one fma per term (the order that defines a problem's bits).  The
// loads of eight categories for all N entries are issued before the first fma, so a lane keeps 8 N loads in flight instead of
// paying one trip to L2 / the Infinity Cache per term.
template <int N>
__device__ __forceinline__ void cv_combine(const double* __restrict__ Sp, int C, const double* __restrict__ base, int64_t T,
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

// Kernel V0: total[c] = sum_f stats[f][c] and rest[f][c] = total[c] - stats[f][c], the term every problem of fold f combines
// (formed once here, so kernel V1 reads one block per term instead of two).  grid (ceil(T / 256), C)
__global__ __launch_bounds__(256) void fsnap_cv_total_k(const double* __restrict__ stats, int F, int C, int K,
                                                        double* __restrict__ total, double* __restrict__ rest) {
    const int64_t T = (int64_t)K * K + K + 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T) return;
    const int c = blockIdx.y;
    double s = stats[(int64_t)c * T + e];
    for (int f = 1; f < F; ++f) s += stats[((int64_t)f * C + c) * T + e];
    total[(int64_t)c * T + e] = s;
    for (int f = 0; f < F; ++f) rest[((int64_t)f * C + c) * T + e] = s - stats[((int64_t)f * C + c) * T + e];
}

// Kernel V1.  coef[p][f][K]; info[p][f][4] = status (0 solved, 1 a pivot of the scaled matrix was not > pivot_tol), smallest
// scaled pivot met (inf without a live column), live columns, sum_c S^2 (T.n - B.n).
__global__ __launch_bounds__(CV_THREADS) void fsnap_cv_solve_k(const double* __restrict__ rest, const double* __restrict__ total,
                                                               const double* __restrict__ S, int P, int F, int C, int K,
                                                               double alpha, double pivot_tol, double* __restrict__ coef_out,
                                                               double* __restrict__ info_out) {
    extern __shared__ __attribute__((aligned(16))) double cv_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t T = (int64_t)K * K + K + 3;
    const int KK = K * K;
    double* tri = cv_lds;                        // packed lower triangle of the live, scaled system; then L (diagonal in dl)
    double* dsc = tri + K * (K + 1) / 2;         // d by column (1 for dead columns)
    double* rhs = dsc + K;                       // qv / d by position, updated by the forward substitution
    double* yv = rhs + K;                        // y of L y = rhs by position, updated by the back substitution
    double* cv0 = yv + K;                        // the scaled column of a step; then x of L^T x = y
    double* dl = cv0 + K;                        // diagonal of L by position
    double* coef = dl + K;                       // coefficients by column
    int* idx = (int*)(coef + K);                 // the live columns in ascending order
    int* flag = idx + K;
    int* cnt = flag + K;
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const int nprob = P * F;
    for (int prob = blockIdx.x; prob < nprob; prob += gridDim.x) {
        const int p = prob / F, f = prob - p * F;
        const double* Sp = S + (int64_t)p * C;
        const double* Rf = rest + (int64_t)f * C * T;     // rest[f][c] = T[c] - B[f][c]
        // live columns: the candidate's total touched the column and the downdate left more than noise
        if (tid < K) {
            const int64_t at[1] = {(int64_t)tid * K + tid};
            double tp[1], q[1];
            cv_combine<1>(Sp, C, total, T, at, tp);
            cv_combine<1>(Sp, C, Rf, T, at, q);
            const bool dead = tp[0] == 0.0 || q[0] <= pivot_tol * tp[0];
            dsc[tid] = dead ? 1.0 : sqrt(q[0] + alpha);
            flag[tid] = dead ? 0 : 1;
            coef[tid] = 0.0;
        }
        __syncthreads();
        if (wave == 0) {                         // ordered compaction: a ballot prefix, not arrival order
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
        // gather, combine and scale: H_ab = (Qm_ab + alpha [a == b]) / (d_a d_b)
        for (int a = wave; a < k; a += CV_WAVES) {
            const int ia = idx[a];
            const double da = dsc[ia];
            if (lane > a) continue;
            // a lane owns the columns lane, lane + 64, lane + 128 of the row (K <= 144): one combine for the three; a column
            // past the diagonal repeats the first one's address and is dropped
            int64_t at[3];
            double v[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int b = lane + 64 * n;
                at[n] = (int64_t)ia * K + idx[b <= a ? b : lane];
            }
            cv_combine<3>(Sp, C, Rf, T, at, v);
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int b = lane + 64 * n;
                if (b > a) break;
                double h = v[n];
                if (b == a) h += alpha;
                tri[cv_tri(a, b)] = h / (da * dsc[idx[b]]);
            }
        }
        if (tid < k) {
            const int ia = idx[tid];
            const int64_t at[1] = {(int64_t)KK + ia};
            double v[1];
            cv_combine<1>(Sp, C, Rf, T, at, v);
            rhs[tid] = v[0] / dsc[ia];
        }
        __syncthreads();
        // Cholesky of the scaled matrix, right-looking; L y = rhs rides along (y_j is final when column j is scaled)
        double minpiv = inf;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
            const double piv = tri[cv_tri(j, j)];
            minpiv = piv < minpiv ? piv : minpiv;
            if (!(piv > pivot_tol)) {            // NaN included; every thread read the same value: a uniform exit
                if (piv != piv) minpiv = piv;
                ok = false;
                break;
            }
            const double ljj = sqrt(piv);
            const double yj = rhs[j] / ljj;
            for (int i = j + 1 + tid; i < k; i += CV_THREADS) {
                const double v = tri[cv_tri(i, j)] / ljj;
                tri[cv_tri(i, j)] = v;
                cv0[i] = v;
                rhs[i] = __builtin_fma(-v, yj, rhs[i]);
            }
            if (tid == 0) {
                dl[j] = ljj;
                yv[j] = yj;
            }
            __syncthreads();
            for (int i = j + 1 + wave; i < k; i += CV_WAVES) {
                const double li = cv0[i];
                double* row = tri + cv_tri(i, 0);
                for (int c = j + 1 + lane; c <= i; c += 64) row[c] = __builtin_fma(-li, cv0[c], row[c]);
            }
            __syncthreads();
        }
        if (ok) {
            // L^T x = y by rows of L from the last: x_i is final once the rows below it are done
            for (int i = k - 1; i >= 0; --i) {
                const double xi = yv[i] / dl[i];
                const double* row = tri + cv_tri(i, 0);
                for (int j = tid; j < i; j += CV_THREADS) yv[j] = __builtin_fma(-row[j], xi, yv[j]);
                if (tid == 0) cv0[i] = xi;
                __syncthreads();
            }
            if (tid < k) {
                const int ia = idx[tid];
                coef[ia] = cv0[tid] / dsc[ia];
            }
        }
        __syncthreads();
        if (tid < K) coef_out[(int64_t)prob * K + tid] = ok ? coef[tid] : nan;
        if (tid == 0) {
            const int64_t at[1] = {(int64_t)KK + K + 2};
            double nw[1];
            cv_combine<1>(Sp, C, Rf, T, at, nw);
            const double n = nw[0];
            double* io = info_out + (int64_t)prob * 4;
            io[0] = ok ? 0.0 : 1.0;
            io[1] = minpiv;
            io[2] = (double)k;
            io[3] = n;
        }
        __syncthreads();                         // the next problem refills the vectors
    }
}

// Kernel V2: each wave takes 16-row blocks of the chunk (block wave, wave + 4, ...).  Forward product y[16 rows][16 candidates]
// with 2 MFMAs per 8 columns: lane (row e, slot ks) holds a[row][k0 + 2 ks + {0, 1}], betaT[fold][k][16] (zero-padded to a
// multiple of 8 rows and to 16 candidates) gives the matching B slots; two 8-column steps are issued together so that four
// loads of a row are in flight.  The result tile holds y[row ks + 4 g][candidate e] in register g; the lane keeps the four
// sums of candidate e; partial[chunk * 4 + wave][4][16].
__global__ __launch_bounds__(256) void fsnap_cv_rows_k(const double* __restrict__ A, int64_t lda, const double* __restrict__ b,
                                                       const double* __restrict__ w0, const int* __restrict__ idx,
                                                       const CatChunk* __restrict__ chunks, int K, int C,
                                                       const double* __restrict__ betaT, double* __restrict__ partial) {
    const int64_t chunk = blockIdx.x;
    const CatChunk ch = chunks[chunk];
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int K8 = (K + 7) / 8 * 8;
    const double* bt = betaT + (int64_t)(ch.cat / C) * K8 * 16;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int nblk = (ch.count + 15) / 16;
    for (int rb = wave; rb < nblk; rb += 4) {
        const int pos = rb * 16 + e;
        const bool valid = pos < ch.count;
        const int r32 = idx[ch.first + (valid ? pos : 0)];
        const double* src = A + (int64_t)r32 * lda;
        d4 y = {0.0, 0.0, 0.0, 0.0};
        int k0 = 0;
        for (; k0 + 16 <= K8; k0 += 16) {
            const int ka = k0 + 2 * ks, kb = ka + 8;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            if (valid && ka < K) a0 = src[ka];
            if (valid && ka + 1 < K) a1 = src[ka + 1];
            if (valid && kb < K) a2 = src[kb];
            if (valid && kb + 1 < K) a3 = src[kb + 1];
            const double b0 = bt[(int64_t)ka * 16 + e], b1 = bt[(int64_t)(ka + 1) * 16 + e];
            const double b2 = bt[(int64_t)kb * 16 + e], b3 = bt[(int64_t)(kb + 1) * 16 + e];
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, y, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, y, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, y, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b3, y, 0, 0, 0);
        }
        if (k0 < K8) {                           // K8 is an odd multiple of 8: one more 8-column step
            const int ka = k0 + 2 * ks;
            double a0 = 0.0, a1 = 0.0;
            if (valid && ka < K) a0 = src[ka];
            if (valid && ka + 1 < K) a1 = src[ka + 1];
            const double b0 = bt[(int64_t)ka * 16 + e], b1 = bt[(int64_t)(ka + 1) * 16 + e];
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, y, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, y, 0, 0, 0);
        }
        const double t = valid ? b[r32] : 0.0, wv = valid ? w0[r32] : 0.0;
        const int vi = valid ? 1 : 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int sl = ks + 4 * g;
            const double tr = __shfl(t, sl, 64), wr = __shfl(wv, sl, 64);
            const bool vr = __shfl(vi, sl, 64) != 0;
            const double res = tr - y[g];
            if (vr) {
                const double wres = wr * res;
                s0 += __builtin_fabs(res);
                s1 = __builtin_fma(res, res, s1);
                s2 += __builtin_fabs(wres);
                s3 = __builtin_fma(wres, wres, s3);
            }
        }
    }
    const int64_t slot = chunk * 4 + wave;
    double v[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = ks_sum(v[q]);
        if (ks == 0) partial[(slot * 4 + q) * 16 + e] = v[q];
    }
}

}  // namespace

size_t cv_lds_bytes(int K) { return ((size_t)K * (K + 1) / 2 + 6 * (size_t)K) * 8 + (2 * (size_t)K + 2) * 4; }

int cv_blocks_per_cu(int K) {
    const size_t per = (size_t)160 * 1024 / (cv_lds_bytes(K) + 512);
    return per < 1 ? 1 : per > 4 ? 4 : (int)per;
}

hipError_t launch_cv_total(const double* stats, int F, int C, int K, double* total, double* rest, hipStream_t st) {
    const int64_t T = (int64_t)K * K + K + 3;
    fsnap_cv_total_k<<<dim3((unsigned)((T + 255) / 256), (unsigned)C), 256, 0, st>>>(stats, F, C, K, total, rest);
    return hipGetLastError();
}

hipError_t launch_cv_solve(int nblocks, const double* rest, const double* total, const double* S, int P, int F, int C, int K,
                           double alpha, double* coef, double* info, hipStream_t st) {
    if (K < 1 || K > CV_MAX_K || nblocks < 1) return hipErrorInvalidValue;
    // set on every launch: the attribute belongs to the current device, and the call costs microseconds next to the kernel
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_cv_solve_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)cv_lds_bytes(CV_MAX_K));
    if (e != hipSuccess) return e;
    fsnap_cv_solve_k<<<dim3((unsigned)nblocks), dim3(CV_THREADS), cv_lds_bytes(K), st>>>(rest, total, S, P, F, C, K, alpha,
                                                                                        LOCO_PIVOT_TOL, coef, info);
    return hipGetLastError();
}

hipError_t launch_cv_rows(const double* A, int64_t lda, const double* b, const double* w0, const int* idx, const CatChunk* chunks,
                          int64_t nchunks, int K, int C, const double* betaT, double* partial, hipStream_t st) {
    if (nchunks <= 0) return hipSuccess;
    fsnap_cv_rows_k<<<dim3((unsigned)nchunks), 256, 0, st>>>(A, lda, b, w0, idx, chunks, K, C, betaT, partial);
    return hipGetLastError();
}

}  // namespace fsnap
