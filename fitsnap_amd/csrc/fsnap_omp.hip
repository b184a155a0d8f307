// fsnap_omp.hip — grouped K-fold greedy forward-selection paths on the per-fold statistics (fsnap_omp_path; the host algebra and
// the tables are solvers/omp_path.py).  Forward selection touches the rows only through (X^T X, X^T y, |y|^2): it is a Cholesky
// factorisation of the downdated matrix "total minus block f" whose pivot is chosen by the selection criterion, with the
// right-hand side carried along, so the F + 1 problems (fold f left out, or none) are independent K x K recurrences on the folds
// and the total of kernel S1 (fsnap_lasso.hip).
//   Kernel O1: one wave per problem, grid-stride.  The factor rows W (S x K, row stride K | 1 so that a column read -- the
//              back substitution's L[v][u] = W[u][j_v] -- touches 32 distinct banks per lane group) sit in LDS; r, t and the
//              diagonal of Qm in registers (lane l owns columns l, l + 64, l + 128); z and beta by step position in LDS.  Per step
//              the pivot row of Qm (K doubles, total row minus fold row) is the only read of the matrix; the held-out form reads
//              the s x s sub-block of G_f on the support.  The recurrence is fsnap_omp_gram's statement for statement
//              (fsnap_solve.cpp), every multiply-add an explicit fma; only the two sums of the held-out form run as wave
//              butterflies.  The argmax compares (score, index) pairs exactly through a butterfly, so any lane layout gives the
//              same column.  fp64 VALU only, no atomics.
// A problem's result depends on its own fold only: bit-identical run to run and under any permutation or subset of the folds.
#include <hip/hip_runtime.h>

#include "fsnap_fold_body.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

constexpr int OMP_CRIT_OLS = 1;

// a[slot] for a uniform slot without indexing the registers dynamically
template <typename V, int NE>
__device__ __forceinline__ V omp_pick(const V (&a)[NE], int slot) {
    V v = a[0];
#pragma unroll
    for (int e = 1; e < NE; ++e)
        if (slot == e) v = a[e];
    return v;
}

// Kernel O1.  NE = ceil(K / 64) columns per lane; step positions lane, lane + 64 (S <= 128).
// LDS: S (K | 1) + 2 S + K doubles (W, z, beta by position, one dense coefficient row) and S ints (the chosen columns).
template <int NE>
__global__ __launch_bounds__(64) void fsnap_omp_path_k(const double* __restrict__ folds, const double* __restrict__ total, int K,
                                                       int F, int criterion, const int* __restrict__ forced, int nforced, int S,
                                                       const int* __restrict__ levels, int Q, double pivot_tol,
                                                       int* __restrict__ order, double* __restrict__ path,
                                                       double* __restrict__ heldout, double* __restrict__ coef) {
    extern __shared__ __attribute__((aligned(16))) double omp_lds[];
    const int lane = threadIdx.x;
    const int64_t T = (int64_t)K * K + K + 3;
    const int KK = K * K;
    const int KP = K | 1;
    double* W = omp_lds;
    double* sz = W + (size_t)S * KP;
    double* sb = sz + S;
    double* sd = sb + S;
    int* so = (int*)(sd + K);
    int col[NE], cidx[NE];
    bool valid[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        col[e] = lane + 64 * e;
        valid[e] = col[e] < K;
        cidx[e] = valid[e] ? col[e] : 0;
    }
    for (int f = blockIdx.x; f <= F; f += gridDim.x) {
        // (fold_view's statements, kept as this kernel's own text: through the shared view the register allocation of O1
        // comes out differently -- two scalar registers fewer spilled --, and the shared pieces are to cost or change nothing)
        const double* Gf = f < F ? folds + (int64_t)f * T : nullptr;
        const double bb_f = Gf ? Gf[KK + K] : 0.0, n_f = Gf ? Gf[KK + K + 2] : 0.0;
        double e_cur = Gf ? total[KK + K] - bb_f : total[KK + K];
        double r[NE], t[NE], qd[NE];
        bool alive[NE], cand[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int j = cidx[e];
            const double tjj = total[(int64_t)j * K + j];
            const double qjj = Gf ? tjj - Gf[(int64_t)j * K + j] : tjj;
            alive[e] = valid[e] && !fold_dead(tjj, qjj, pivot_tol);
            cand[e] = alive[e];
            qd[e] = alive[e] ? qjj : 0.0;
            t[e] = qd[e];
            double v = 0.0;
            if (alive[e]) v = Gf ? total[KK + j] - Gf[KK + j] : total[KK + j];
            r[e] = v;
        }
        int fpos = 0, ns = 0, qi = 0;
        bool ended = false;
        double h_last = bb_f;
        for (int s = 0; s < S; ++s) {
            int js = -1;
            double sc_out = 0.0, pv_out = 0.0;
            if (!ended) {
                // a candidate inside the span of the support is struck for the rest of the problem
                unsigned long long cm[NE];
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    if (cand[e] && t[e] <= pivot_tol * qd[e]) cand[e] = false;
                    cm[e] = __ballot(cand[e]);
                }
                while (fpos < nforced && js < 0) {
                    const int j = forced[fpos++];
                    if ((omp_pick(cm, j >> 6) >> (j & 63)) & 1ull) js = j;
                }
                if (js < 0) {
                    // exact argmax of the fp64 scores, the lowest index on equality (a lane's columns ascend with e)
                    double bs = -1.0;
                    int bj = 0x7FFFFFFF;
#pragma unroll
                    for (int e = 0; e < NE; ++e)
                        if (cand[e]) {
                            const double sc = r[e] * r[e] / (criterion == OMP_CRIT_OLS ? t[e] : qd[e]);
                            if (sc > bs) {
                                bs = sc;
                                bj = col[e];
                            }
                        }
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const double os = __shfl_xor(bs, o, 64);
                        const int oj = __shfl_xor(bj, o, 64);
                        if (os > bs || (os == bs && oj < bj)) {
                            bs = os;
                            bj = oj;
                        }
                    }
                    if (bj != 0x7FFFFFFF) js = bj;
                }
                if (js < 0) ended = true;
            }
            if (js >= 0) {
                const int ol = js & 63, oe = js >> 6;
                const double tj = lane_bcast(omp_pick(t, oe), ol);
                const double rj = lane_bcast(omp_pick(r, oe), ol);
                const double qj = lane_bcast(omp_pick(qd, oe), ol);
                const double l = sqrt(tj);
                const double z = rj / l;
                sc_out = rj * rj / (criterion == OMP_CRIT_OLS ? tj : qj);
                pv_out = tj;
                // the pivot row of Qm, left-looking: minus what the earlier rows of W already explain
                const double* trow = total + (int64_t)js * K;
                const double* grow = Gf ? Gf + (int64_t)js * K : nullptr;
                double acc[NE];
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    double v = 0.0;
                    if (alive[e]) v = grow ? trow[cidx[e]] - grow[cidx[e]] : trow[cidx[e]];
                    acc[e] = v;
                }
#pragma unroll 4
                for (int u = 0; u < ns; ++u) {
                    const double* wu = W + (size_t)u * KP;
                    const double a = wu[js];
#pragma unroll
                    for (int e = 0; e < NE; ++e) acc[e] = __builtin_fma(-a, wu[cidx[e]], acc[e]);
                }
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const double w = alive[e] ? acc[e] / l : 0.0;
                    if (valid[e]) W[(size_t)ns * KP + col[e]] = w;
                    r[e] = __builtin_fma(-w, z, r[e]);
                    t[e] = __builtin_fma(-w, w, t[e]);
                    if (col[e] == js) cand[e] = false;
                }
                e_cur = __builtin_fma(-z, z, e_cur);
                if (lane == 0) {
                    sz[ns] = z;
                    so[ns] = js;
                }
                ++ns;
                __syncthreads();
                // L^T beta = z, L[v][u] = W[u][j_v]: column-oriented back substitution from the last row up
                double x[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) x[i] = lane + 64 * i < ns ? sz[lane + 64 * i] : 0.0;
                for (int v = ns - 1; v >= 0; --v) {
                    const int jv = so[v];
                    const double bv = lane_bcast(v < 64 ? x[0] : x[1], v & 63) / W[(size_t)v * KP + jv];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int p = lane + 64 * i;
                        if (p < v)
                            x[i] = __builtin_fma(-W[(size_t)p * KP + jv], bv, x[i]);
                        else if (p == v)
                            x[i] = bv;
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    if (lane + 64 * i < ns) sb[lane + 64 * i] = x[i];
                __syncthreads();
                if (Gf) {
                    // weighted squared error of fold f under its own refit: bb_f - 2 beta . c_f + beta^T G_f beta on the support
                    double a[2] = {0.0, 0.0};
                    const double* row[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) row[i] = Gf + (int64_t)(lane + 64 * i < ns ? so[lane + 64 * i] : 0) * K;
                    // (unrolled so that several gathers from L2 are in flight; the sums still run with u ascending)
#pragma unroll 8
                    for (int u = 0; u < ns; ++u) {
                        const int ju = so[u];
                        const double bu = sb[u];
#pragma unroll
                        for (int i = 0; i < 2; ++i)
                            if (lane + 64 * i < ns) a[i] = __builtin_fma(row[i][ju], bu, a[i]);
                    }
                    double s1 = 0.0, s2 = 0.0;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        if (lane + 64 * i < ns) {
                            s1 = __builtin_fma(x[i], Gf[KK + so[lane + 64 * i]], s1);
                            s2 = __builtin_fma(x[i], a[i], s2);
                        }
                    s1 = wave_sum(s1);
                    s2 = wave_sum(s2);
                    h_last = bb_f - 2.0 * s1 + s2;
                }
            }
            // the records of step s; once the path has ended they repeat the last step's
            if (lane == 0) {
                const int64_t at = (int64_t)f * S + s;
                order[at] = js;
                path[at * 3 + 0] = e_cur;
                path[at * 3 + 1] = sc_out;
                path[at * 3 + 2] = pv_out;
                if (Gf) fold_heldout_store(heldout + at * 3, n_f, h_last, bb_f);
            }
            if (qi < Q && levels[qi] == s + 1) {
                // the dense coefficient row through LDS, so that every global entry is written once
#pragma unroll
                for (int e = 0; e < NE; ++e)
                    if (valid[e]) sd[col[e]] = 0.0;
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    if (lane + 64 * i < ns) sd[so[lane + 64 * i]] = sb[lane + 64 * i];
                __syncthreads();
                while (qi < Q && levels[qi] == s + 1) {
#pragma unroll
                    for (int e = 0; e < NE; ++e)
                        if (valid[e]) coef[((int64_t)f * Q + qi) * K + col[e]] = sd[col[e]];
                    ++qi;
                }
                __syncthreads();
            }
        }
        __syncthreads();                                       // the next problem rewrites W, z and the chosen columns
    }
}

}  // namespace

size_t omp_lds_bytes(int K, int S) {
    const size_t bytes = ((size_t)S * (size_t)(K | 1) + 2 * (size_t)S + (size_t)K) * 8 + (size_t)S * 4;
    return (bytes + 15) & ~(size_t)15;
}

int omp_blocks_per_cu(int K, int S) {
    const size_t per = (size_t)160 * 1024 / (omp_lds_bytes(K, S) + 512);
    return per < 1 ? 1 : per > 8 ? 8 : (int)per;
}

template <int NE>
static hipError_t omp_path_launch(int nblocks, size_t lds, const double* folds, const double* total, int K, int F, int criterion,
                                  const int* forced, int nforced, int S, const int* levels, int Q, int* order, double* path,
                                  double* heldout, double* coef, hipStream_t st) {
    // set on every launch: the attribute belongs to the current device, and the call costs microseconds next to the kernel
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_omp_path_k<NE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)omp_lds_bytes(64 * NE < OMP_MAX_K ? 64 * NE : OMP_MAX_K, OMP_MAX_S));
    if (e != hipSuccess) return e;
    fsnap_omp_path_k<NE><<<dim3((unsigned)nblocks), dim3(64), lds, st>>>(folds, total, K, F, criterion, forced, nforced, S, levels,
                                                                         Q, LOCO_PIVOT_TOL, order, path, heldout, coef);
    return hipGetLastError();
}

hipError_t launch_omp_path(int nblocks, const double* folds, const double* total, int K, int F, int criterion, const int* forced,
                           int nforced, int S, const int* levels, int Q, int* order, double* path, double* heldout, double* coef,
                           hipStream_t st) {
    if (K < 1 || K > OMP_MAX_K || S < 1 || S > OMP_MAX_S || S > K || nblocks < 1 || Q < 1 || nforced < 0) return hipErrorInvalidValue;
    const size_t lds = omp_lds_bytes(K, S);
    switch ((K + 63) / 64) {
        case 1:
            return omp_path_launch<1>(nblocks, lds, folds, total, K, F, criterion, forced, nforced, S, levels, Q, order, path, heldout,
                                      coef, st);
        case 2:
            return omp_path_launch<2>(nblocks, lds, folds, total, K, F, criterion, forced, nforced, S, levels, Q, order, path, heldout,
                                      coef, st);
        default:
            return omp_path_launch<3>(nblocks, lds, folds, total, K, F, criterion, forced, nforced, S, levels, Q, order, path, heldout,
                                      coef, st);
    }
}

}  // namespace fsnap
