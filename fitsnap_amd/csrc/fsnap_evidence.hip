// fsnap_evidence.hip — marginal likelihood of group-weight candidates from the per-category statistics
// (fsnap_candidates_evidence; the definitions, the host assembly and the ascent are solvers/candidates_evidence.py).  gfx950 only.
//
// The context holds C packed blocks B[c] = [G | r | bb, sum wb, n] (fsnap_cat_normal_eq).  Candidate p scales category c by
// S[p, c] (0 for the categories that take no part: the caller masks them).  Per candidate, on the live columns,
//     H = sum_c S[p,c]^2 B[c].G + alpha I,  beta = H^-1 sum_c S[p,c]^2 B[c].r,  log|H|,  H^-1
// and per (candidate, category) the two inner products of the block with [H^-1 | 0 | 0,0,0] and [beta beta' | -2 beta | 1,0,0]:
//     T[p][c] = tr(H^-1 B[c].G),   Q[p][c] = bb_c - 2 beta . r_c + beta' G_c beta.
//   E1  fsnap_evidence_factor_k  one workgroup of 256 threads per candidate, grid-stride.  Kernel V1's body (fsnap_cv.hip: the
//                                combination over c, live rule, Jacobi scaling, right-looking Cholesky with the forward
//                                substitution riding along, back substitution, pivot tolerance) as this kernel's own copy, then
//                                log|H| = 2 sum_j (log l_jj + log d_j) on one lane, j ascending, and the inverse IN PLACE on the
//                                packed triangle in LDS (no second triangle fits: K = 144 takes 83 520 B): L -> X = L^-1 by
//                                columns from the last (column j of X is -X[j+1:, j+1:] L[j+1:, j] / l_jj, one thread per row, m
//                                ascending), then X'X by rows from the first (row a needs the rows >= a of X only, one thread per
//                                entry, i ascending), un-scaled by 1 / (d_a d_b) on the way out.  It writes beta, the scalars and
//                                the two table columns of its candidate, tab[p / 8][e][2 (p % 8) + {0, 1}], e < K^2 + K + 3.
//   E2  fsnap_evidence_sweep_k   one wave per (tile of 16 categories, tile of 8 candidates = 16 table columns, slice of 512
//                                elements): Y = blocks . table on v_mfma_f64_16x16x4_f64, lane (e, ks) holding the elements
//                                k0 + 2 ks + {0, 1} of block 16 ct + e and the matching table slots of column e, two MFMAs per 8
//                                elements, k0 ascending.  Categories past C and elements past the block end are zero-filled,
//                                not read.
//   E3  fsnap_evidence_reduce_k  adds the slices of every (category, column) in slice order.
// fp64, no atomics.  Every sum runs in an order fixed by K and C alone; a candidate is one pair of MFMA columns and no other
// column enters it: a candidate's bits do not depend on the batch, the grid or the run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fsnap_device_common.h"
#include "fsnap_kernels.h"

namespace fsnap {
namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;

__device__ __forceinline__ int ev_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// kernel V1's combination (c ascending, one fma per term, the loads of eight categories in flight)
template <int N>
__device__ __forceinline__ void ev_combine(const double* __restrict__ Sp, int C, const double* __restrict__ base, int64_t T,
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

// Kernel E1.  beta[p][K] (NaN with status 1); info[p][6] = status (0 solved, 1 a pivot of the scaled matrix was not > pivot_tol),
// smallest scaled pivot met (inf without a live column), live columns, log|H|, tr(H^-1), 0; the candidate's two table columns
// (all zeros with status 1).
__global__ __launch_bounds__(EV_THREADS) void fsnap_evidence_factor_k(const double* __restrict__ stats, const double* __restrict__ S,
                                                                      int P, int C, int K, double alpha, double pivot_tol,
                                                                      double* __restrict__ beta_out, double* __restrict__ info_out,
                                                                      double* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) double ev_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t T = (int64_t)K * K + K + 3;
    const int KK = K * K;
    double* tri = ev_lds;                        // the layout of kernel V1 (cv_lds_bytes)
    double* dsc = tri + K * (K + 1) / 2;         // d by column (1 for dead columns)
    double* rhs = dsc + K;
    double* yv = rhs + K;
    double* cv0 = yv + K;                        // the column of a step, here also of the two inversion sweeps
    double* dl = cv0 + K;                        // diagonal of L by position
    double* coef = dl + K;                       // coefficients by column
    int* idx = (int*)(coef + K);                 // the live columns in ascending order
    int* flag = idx + K;                         // live flag, then position + 1 of a live column (0: dead)
    int* cnt = flag + K;
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        const double* Sp = S + (int64_t)p * C;
        if (tid < K) {
            const int64_t at[1] = {(int64_t)tid * K + tid};
            double tp[1];
            ev_combine<1>(Sp, C, stats, T, at, tp);
            const bool dead = tp[0] == 0.0;
            dsc[tid] = dead ? 1.0 : sqrt(tp[0] + alpha);
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
        if (tid < k) flag[idx[tid]] = tid + 1;   // read again only after the barriers below
        for (int a = wave; a < k; a += EV_WAVES) {
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
            ev_combine<3>(Sp, C, stats, T, at, v);
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int b = lane + 64 * n;
                if (b > a) break;
                double h = v[n];
                if (b == a) h += alpha;
                tri[ev_tri(a, b)] = h / (da * dsc[idx[b]]);
            }
        }
        if (tid < k) {
            const int ia = idx[tid];
            const int64_t at[1] = {(int64_t)KK + ia};
            double v[1];
            ev_combine<1>(Sp, C, stats, T, at, v);
            rhs[tid] = v[0] / dsc[ia];
        }
        __syncthreads();
        double minpiv = inf;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
            const double piv = tri[ev_tri(j, j)];
            minpiv = piv < minpiv ? piv : minpiv;
            if (!(piv > pivot_tol)) {            // NaN included; every thread read the same value: a uniform exit
                if (piv != piv) minpiv = piv;
                ok = false;
                break;
            }
            const double ljj = sqrt(piv);
            const double yj = rhs[j] / ljj;
            for (int i = j + 1 + tid; i < k; i += EV_THREADS) {
                const double v = tri[ev_tri(i, j)] / ljj;
                tri[ev_tri(i, j)] = v;
                cv0[i] = v;
                rhs[i] = __builtin_fma(-v, yj, rhs[i]);
            }
            if (tid == 0) {
                dl[j] = ljj;
                yv[j] = yj;
            }
            __syncthreads();
            for (int i = j + 1 + wave; i < k; i += EV_WAVES) {
                const double li = cv0[i];
                double* row = tri + ev_tri(i, 0);
                for (int c = j + 1 + lane; c <= i; c += 64) row[c] = __builtin_fma(-li, cv0[c], row[c]);
            }
            __syncthreads();
        }
        double logdet = 0.0, trinv = 0.0;
        if (ok) {
            for (int i = k - 1; i >= 0; --i) {
                const double xi = yv[i] / dl[i];
                const double* row = tri + ev_tri(i, 0);
                for (int j = tid; j < i; j += EV_THREADS) yv[j] = __builtin_fma(-row[j], xi, yv[j]);
                if (tid == 0) cv0[i] = xi;
                __syncthreads();
            }
            if (tid < k) {
                const int ia = idx[tid];
                coef[ia] = cv0[tid] / dsc[ia];
                tri[ev_tri(tid, tid)] = dl[tid]; // the factor's diagonal joins the triangle
            }
            __syncthreads();
            // X = L^-1 in place, columns from the last: the rows and columns past j already hold X
            for (int j = k - 1; j >= 0; --j) {
                const double ljj = tri[ev_tri(j, j)];
                for (int i = j + 1 + tid; i < k; i += EV_THREADS) cv0[i] = tri[ev_tri(i, j)];
                __syncthreads();
                const int i = j + 1 + tid;       // k - j - 1 <= 143 rows: one thread each
                if (i < k) {
                    const double* row = tri + ev_tri(i, 0);
                    double s = 0.0;
                    for (int m = j + 1; m <= i; ++m) s = __builtin_fma(row[m], cv0[m], s);
                    tri[ev_tri(i, j)] = -s / ljj;
                }
                if (tid == EV_THREADS - 1) tri[ev_tri(j, j)] = 1.0 / ljj;
                __syncthreads();
            }
            // W = X' X in place, rows from the first: row a needs the rows >= a of X
            for (int a = 0; a < k; ++a) {
                for (int i = a + tid; i < k; i += EV_THREADS) cv0[i] = tri[ev_tri(i, a)];
                __syncthreads();
                if (tid <= a) {
                    double s = 0.0;
                    for (int i = a; i < k; ++i) s = __builtin_fma(cv0[i], tri[ev_tri(i, tid)], s);
                    tri[ev_tri(a, tid)] = s;
                }
                __syncthreads();
            }
            if (tid == 0) {
                for (int j = 0; j < k; ++j) {
                    const double d = dsc[idx[j]];
                    logdet += log(dl[j]) + log(d);
                    trinv += tri[ev_tri(j, j)] / (d * d);
                }
                logdet *= 2.0;
            }
        }
        __syncthreads();
        if (tid < K) beta_out[(int64_t)p * K + tid] = ok ? coef[tid] : nan;
        if (tid == 0) {
            double* io = info_out + (int64_t)p * 6;
            io[0] = ok ? 0.0 : 1.0;
            io[1] = minpiv;
            io[2] = (double)k;
            io[3] = ok ? logdet : nan;
            io[4] = ok ? trinv : nan;
            io[5] = 0.0;
        }
        // the candidate's two columns of its tile's table: [H^-1 scattered to K x K | 0 | 0, 0, 0] and [beta beta' | -2 beta | 1, 0, 0]
        double* tp = tab + (int64_t)(p >> 3) * T * 16 + 2 * (p & 7);
        for (int e = tid; e < (int)T; e += EV_THREADS) {
            double v0 = 0.0, v1 = 0.0;
            if (ok) {
                if (e < KK) {
                    const int i = e / K, j = e - i * K;
                    const int pi = flag[i], pj = flag[j];
                    if (pi != 0 && pj != 0) {
                        const int a = (pi > pj ? pi : pj) - 1, b = (pi > pj ? pj : pi) - 1;
                        v0 = tri[ev_tri(a, b)] / (dsc[i] * dsc[j]);
                    }
                    v1 = coef[i] * coef[j];
                } else if (e < KK + K) {
                    v1 = -2.0 * coef[e - KK];
                } else if (e == KK + K) {
                    v1 = 1.0;
                }
            }
            tp[(int64_t)e * 16] = v0;
            tp[(int64_t)e * 16 + 1] = v1;
        }
        __syncthreads();                         // the next candidate refills the vectors
    }
}

// Kernel E2.  grid (CT, PT, nslice), CT = ceil(C / 16), PT = ceil(P / 8): part[((ct PT + pt) nslice + s) 4 + g][64 lanes], register g
// of lane (e, ks) holding the partial of category 16 ct + ks + 4 g and table column e.
__global__ __launch_bounds__(64) void fsnap_evidence_sweep_k(const double* __restrict__ stats, const double* __restrict__ tab, int C,
                                                             int K, double* __restrict__ part) {
    const int lane = threadIdx.x, e = lane & 15, ks = lane >> 4;
    const int ct = blockIdx.x, pt = blockIdx.y, s = blockIdx.z;
    const int T = K * K + K + 3;
    const int c = ct * 16 + e;
    const bool cvalid = c < C;
    const double* blk = stats + (int64_t)(cvalid ? c : 0) * T;
    const double* tb = tab + (int64_t)pt * T * 16 + e;
    const int e0 = s * EV_SLICE, e1 = e0 + EV_SLICE < T ? e0 + EV_SLICE : T;
    d4 y = {0.0, 0.0, 0.0, 0.0};
    int k0 = e0;
    for (; k0 + 32 <= e1; k0 += 32) {            // four full steps: their sixteen loads are issued before the first MFMA
        double a[8], b[8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ka = k0 + 8 * u + 2 * ks;
            a[2 * u] = cvalid ? blk[ka] : 0.0;
            a[2 * u + 1] = cvalid ? blk[ka + 1] : 0.0;
            b[2 * u] = tb[(int64_t)ka * 16];
            b[2 * u + 1] = tb[(int64_t)(ka + 1) * 16];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) y = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], y, 0, 0, 0);
    }
    for (; k0 < e1; k0 += 8) {
        const int ka = k0 + 2 * ks;
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
        if (ka < e1) {
            b0 = tb[(int64_t)ka * 16];
            if (cvalid) a0 = blk[ka];
        }
        if (ka + 1 < e1) {
            b1 = tb[(int64_t)(ka + 1) * 16];
            if (cvalid) a1 = blk[ka + 1];
        }
        y = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, y, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, y, 0, 0, 0);
    }
    double* out = part + (((int64_t)ct * gridDim.y + pt) * gridDim.z + s) * 256;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[g * 64 + lane] = y[g];
}

// Kernel E3.  grid (CT PT), 256 threads: thread (g, lane) adds the slices of its entry in slice order; Y[pt][c][16].
__global__ __launch_bounds__(256) void fsnap_evidence_reduce_k(const double* __restrict__ part, int C, int PT, int nslice,
                                                               double* __restrict__ Y) {
    const int tid = threadIdx.x, g = tid >> 6, lane = tid & 63;
    const int ct = blockIdx.x / PT, pt = blockIdx.x - ct * PT;
    const double* src = part + (int64_t)blockIdx.x * nslice * 256 + tid;
    double v = src[0];
    for (int s = 1; s < nslice; ++s) v += src[(int64_t)s * 256];
    const int c = ct * 16 + (lane >> 4) + 4 * g;
    if (c < C) Y[((int64_t)pt * C + c) * 16 + (lane & 15)] = v;
}

}  // namespace

int evidence_slices(int K) { return (K * K + K + 3 + EV_SLICE - 1) / EV_SLICE; }

hipError_t launch_evidence_factor(int nblocks, const double* stats, const double* S, int P, int C, int K, double alpha, double* beta,
                                  double* info, double* tab, hipStream_t st) {
    if (K < 1 || K > CV_MAX_K || nblocks < 1 || P < 1 || C < 1) return hipErrorInvalidValue;
    // set on every launch: the attribute belongs to the current device
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_evidence_factor_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)cv_lds_bytes(CV_MAX_K));
    if (e != hipSuccess) return e;
    fsnap_evidence_factor_k<<<dim3((unsigned)nblocks), dim3(EV_THREADS), cv_lds_bytes(K), st>>>(stats, S, P, C, K, alpha,
                                                                                                LOCO_PIVOT_TOL, beta, info, tab);
    return hipGetLastError();
}

hipError_t launch_evidence_sweep(const double* stats, const double* tab, int P, int C, int K, double* part, double* Y,
                                 hipStream_t st) {
    if (K < 1 || K > CV_MAX_K || P < 1 || C < 1) return hipErrorInvalidValue;
    const int CT = (C + 15) / 16, PT = (P + 7) / 8, ns = evidence_slices(K);
    if (PT > 65535 || (int64_t)CT * PT > 0x7FFFFFFF) return hipErrorInvalidValue;
    fsnap_evidence_sweep_k<<<dim3((unsigned)CT, (unsigned)PT, (unsigned)ns), 64, 0, st>>>(stats, tab, C, K, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    fsnap_evidence_reduce_k<<<dim3((unsigned)(CT * PT)), 256, 0, st>>>(part, C, PT, ns, Y);
    return hipGetLastError();
}

}  // namespace fsnap
