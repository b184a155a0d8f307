// fsnap_spectral.hip — grouped K-fold spectral paths on the per-fold statistics (fsnap_spectral_path; the grid, the host route,
// the picks and the tables are solvers/spectral_path.py).  With one packed block [G | c | bb, sum wb, n] per (fold, row class)
// (fsnap_cat_normal_eq; summed by kernel S1 of fsnap_lasso.hip) the training system of fold f is "total minus fold f", and ONE
// symmetric eigendecomposition Qm[L, L] = V diag(lambda) V^T of its live columns L gives every ridge penalty alpha and every
// singular-value cut rcond as a filter on (lambda, z = V^T qv): beta = V g, g_i = z_i / (lambda_i + alpha) where lambda_i > cut.
//   Kernel E1: one workgroup of 1024 threads per problem (F + 1 of them), grid-stride.  Two-sided Jacobi under the round-robin
//              ordering of fsnap_spectral_body.h: a round holds n / 2 disjoint pairs, thread k < n / 2 forms rotation k from the
//              matrix before the round and updates its own diagonal block, then the workgroup updates the 2 x 2 blocks
//              J_a^T B J_b below the diagonal of pairs (each touches four entries nobody else touches) and the two rows per pair
//              of the eigenvector array -- two barriers per round.  The working matrix is the PACKED LOWER TRIANGLE in LDS
//              (K (K + 1) / 2 doubles: 83.5 KB at K = 144; the full matrix, 162 KiB, would not fit the 160 KiB of a CU).  The
//              eigenvectors (rows, n x n) are in LDS too while triangle + vectors stay within 156 KiB (K <= 113) and otherwise
//              in a per-workgroup scratch in global memory that stays in L2 (K = 144: 166 KB per resident workgroup).
//   Kernel E2: one workgroup per (problem, slice of 16 settings).  g for the slice, then thread j forms beta_j = sum_i g_i V_ij
//              of the 16 settings with one read of V; for f < F thread i forms row i of G_{f,s} beta with one read of the
//              (symmetric) block per slice and class, and thread q sums setting q's record in index order.
// fp64 VALU only, no atomics, plain vector stores.  Every sum runs in an order fixed by the problem and the setting alone: a
// result is bit-identical run to run and under any permutation or subset of the grid or of the folds.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fsnap_fold_body.h"
#include "fsnap_kernels.h"
#include "fsnap_spectral_body.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

constexpr int SPEC_THREADS = SPEC_LANES;
constexpr int SPEC_WAVES = SPEC_THREADS / 64;
constexpr int SPEC_HALF = (SPEC_MAX_K + 1) / 2;                // pairs of a round
constexpr size_t SPEC_LDS_BUDGET = (size_t)156 * 1024;
constexpr int SPEC_BLOCKS_PER_THREAD = (SPEC_HALF * (SPEC_HALF - 1) / 2 + SPEC_THREADS - 1) / SPEC_THREADS;   // 3

__host__ __device__ constexpr size_t spec_fixed_doubles(int K) {
    // triangle, c, s, lambda, qv, the reduction slots
    return (size_t)K * (K + 1) / 2 + 2 * SPEC_HALF + 2 * (size_t)K + 2 * SPEC_WAVES;
}
__host__ __device__ constexpr size_t spec_int_count(int K) { return 3 * (size_t)K + 2 * SPEC_HALF; }   // live, cpos, ord, pp, qq
__host__ __device__ constexpr bool spec_vec_in_lds(int K) {
    return (spec_fixed_doubles(K) + (size_t)K * K) * 8 + spec_int_count(K) * 4 <= SPEC_LDS_BUDGET;
}

// (sum of a, sum of b) over the workgroup: the butterfly in each wave, then the waves in index order.  Two barriers.
__device__ __forceinline__ void block_sum2(double* red, double& a, double& b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        red[wave] = a;
        red[SPEC_WAVES + wave] = b;
    }
    __syncthreads();
    a = red[0];
    b = red[SPEC_WAVES];
#pragma unroll
    for (int w = 1; w < SPEC_WAVES; ++w) {
        a += red[w];
        b += red[SPEC_WAVES + w];
    }
    __syncthreads();                                                  // red is free again
}

// Kernel E1.  vwork: gridDim.x x K^2 doubles (used where the eigenvectors do not fit LDS).  eig, z: [F + 1][K] ascending, zero
// past n_live; V: [F + 1][K][K], row r < n_live = eigenvector r in the K original coordinates (0 on dead columns); info[F + 1][6].
__global__ __launch_bounds__(SPEC_THREADS) void fsnap_spectral_eig_k(const double* __restrict__ folds,
                                                                     const double* __restrict__ total, int K, int F,
                                                                     double pivot_tol, double* __restrict__ vwork,
                                                                     double* __restrict__ eig, double* __restrict__ z,
                                                                     double* __restrict__ V, double* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double spec_lds[];
    const int tid = threadIdx.x;
    const int KK = K * K;
    double* tri = spec_lds;
    double* cs = tri + (size_t)K * (K + 1) / 2;
    double* sn = cs + SPEC_HALF;
    double* lam = sn + SPEC_HALF;
    double* qv = lam + K;
    double* red = qv + K;
    double* vl = red + 2 * SPEC_WAVES;                                // K^2 doubles where they fit
    const bool in_lds = spec_vec_in_lds(K);
    int* live = (int*)(in_lds ? vl + (size_t)K * K : vl);             // compact -> original column
    int* cpos = live + K;                                             // original -> compact, -1: dead
    int* ord = cpos + K;                                              // sorted -> position on the diagonal
    int* pp = ord + K;
    int* qq = pp + SPEC_HALF;
    double* W = in_lds ? vl : vwork + (size_t)blockIdx.x * KK;        // the eigenvectors as rows, n x n

    for (int p = blockIdx.x; p <= F; p += gridDim.x) {
        const FoldView fv = fold_view(folds, total, p, F, K);
        const double* Gf = fv.Gf;
        auto qm = [&](int r, int c) {
            const int64_t at = (int64_t)r * K + c;
            return Gf ? total[at] - Gf[at] : total[at];
        };
        // the live columns, compacted in index order
        if (tid < K) cpos[tid] = fold_dead(total[(int64_t)tid * K + tid], qm(tid, tid), pivot_tol) ? -1 : 0;
        __syncthreads();
        int n = 0, mine = 0;
        for (int j = 0; j < K; ++j) {
            const int a = cpos[j] >= 0 ? 1 : 0;
            mine += j < tid ? a : 0;
            n += a;
        }
        const bool alive = tid < K && cpos[tid] >= 0;
        __syncthreads();
        if (tid < K) {
            if (alive) {
                cpos[tid] = mine;
                live[mine] = tid;
                qv[mine] = Gf ? total[KK + tid] - Gf[KK + tid] : total[KK + tid];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < n * n; idx += SPEC_THREADS) {
            const int i = idx / n, j = idx - i * n;
            if (j <= i) tri[spec_tri(i, j)] = qm(live[i], live[j]);
            W[idx] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        const int m = n + (n & 1), h = m / 2, nblk = h * (h - 1) / 2;
        const int lane = tid & 63, wave = tid >> 6;
        int ba[SPEC_BLOCKS_PER_THREAD], bb[SPEC_BLOCKS_PER_THREAD];  // this thread's blocks (a, b), b < a; a = 0: none
#pragma unroll
        for (int u = 0; u < SPEC_BLOCKS_PER_THREAD; ++u) {
            const int e = tid + u * SPEC_THREADS;
            ba[u] = e < nblk ? spec_block_row(e) : 0;
            bb[u] = e - ba[u] * (ba[u] - 1) / 2;
        }
        int sweeps = 0, status = 0;
        double off2 = 0.0, diag2 = 0.0;
        for (;;) {
            off2 = 0.0;
            diag2 = 0.0;
            for (int idx = tid; idx < n * n; idx += SPEC_THREADS) {
                const int i = idx / n, j = idx - i * n;
                if (j > i) continue;
                const double a = tri[spec_tri(i, j)];
                if (j == i)
                    diag2 = fma(a, a, diag2);
                else
                    off2 = fma(a, a, off2);
            }
            block_sum2(red, off2, diag2);
            if (off2 == 0.0 || off2 <= SPEC_STOP * diag2) break;
            if (sweeps == SPEC_MAX_SWEEPS) {
                status = 2;
                break;
            }
            for (int r = 0; r < m - 1; ++r) {
                if (tid < h) {                                        // the rotations of the round, from the matrix before it
                    int a, b;
                    spec_pair(m, r, tid, a, b);
                    pp[tid] = a;
                    qq[tid] = b < n ? b : -1;
                    double c = 1.0, s = 0.0;
                    if (b < n) {
                        const int ipp = spec_tri(a, a), iqq = spec_tri(b, b), ipq = spec_tri(b, a);
                        const double app = tri[ipp], aqq = tri[iqq], apq = tri[ipq];
                        const SpecRot rot = spec_rot(app, aqq, apq);
                        c = rot.c;
                        s = rot.s;
                        tri[ipp] = fma(-rot.t, apq, app);
                        tri[iqq] = fma(rot.t, apq, aqq);
                        tri[ipq] = 0.0;
                    }
                    cs[tid] = c;
                    sn[tid] = s;
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < SPEC_BLOCKS_PER_THREAD; ++u) {    // the blocks below the diagonal of pairs
                    const int a = ba[u], b = bb[u];
                    if (a == 0) continue;
                    const double sa = sn[a], sb = sn[b];
                    if (sa == 0.0 && sb == 0.0) continue;
                    const int pa = pp[a], qa = qq[a], pb = pp[b], qb = qq[b];
                    const int i00 = spec_tri(pa, pb), i01 = qb >= 0 ? spec_tri(pa, qb) : -1, i10 = qa >= 0 ? spec_tri(qa, pb) : -1;
                    const int i11 = (qa >= 0 && qb >= 0) ? spec_tri(qa, qb) : -1;
                    double b00 = tri[i00], b01 = i01 >= 0 ? tri[i01] : 0.0, b10 = i10 >= 0 ? tri[i10] : 0.0;
                    double b11 = i11 >= 0 ? tri[i11] : 0.0;
                    spec_block(cs[a], sa, cs[b], sb, b00, b01, b10, b11);
                    tri[i00] = b00;
                    if (i01 >= 0) tri[i01] = b01;
                    if (i10 >= 0) tri[i10] = b10;
                    if (i11 >= 0) tri[i11] = b11;
                }
                for (int k = wave; k < h; k += SPEC_WAVES) {          // eigenvectors: a wave takes the two rows of a pair
                    const double s = sn[k];
                    if (s == 0.0) continue;                           // a bye has s = 0 too
                    const double c = cs[k];
                    double* vp = W + (size_t)pp[k] * n;
                    double* vq = W + (size_t)qq[k] * n;
                    for (int e = lane; e < n; e += 64) {
                        double x = vp[e], y = vq[e];
                        spec_apply(c, s, x, y);
                        vp[e] = x;
                        vq[e] = y;
                    }
                }
                __syncthreads();
            }
            ++sweeps;
        }
        // ascending by (lambda, position on the diagonal)
        double li = 0.0;
        if (tid < n) {
            li = tri[spec_tri(tid, tid)];
            lam[tid] = li;
        }
        __syncthreads();
        double lmax = 0.0, lmin = 0.0;
        int rk = 0;
        for (int j = 0; j < n; ++j) {
            const double lj = lam[j];
            if (lj < li || (lj == li && j < tid)) ++rk;
            lmax = fabs(lj) > lmax ? fabs(lj) : lmax;
            lmin = (j == 0 || lj < lmin) ? lj : lmin;
        }
        if (tid < n) ord[rk] = tid;
        if (tid < K) {
            if (tid < n) eig[(int64_t)p * K + rk] = li;
            if (tid >= n) eig[(int64_t)p * K + tid] = 0.0;
        }
        __syncthreads();
        if (tid < K) {
            double acc = 0.0;
            if (tid < n) {
                const double* v = W + (size_t)ord[tid] * n;
                for (int c = 0; c < n; ++c) acc = fma(v[c], qv[c], acc);
            }
            z[(int64_t)p * K + tid] = acc;
        }
        double* Vp = V + (int64_t)p * KK;
        for (int idx = tid; idx < n * K; idx += SPEC_THREADS) {
            const int r = idx / K, j = idx - r * K;
            const int c = cpos[j];
            Vp[idx] = c >= 0 ? W[(size_t)ord[r] * n + c] : 0.0;
        }
        if (tid == 0) {
            double* io = info + (int64_t)p * 6;
            io[0] = (double)n;
            io[1] = (double)sweeps;
            io[2] = diag2 > 0.0 ? sqrt(off2 / diag2) : 0.0;
            io[3] = lmax;
            io[4] = lmin;
            io[5] = (double)status;
        }
        __syncthreads();                                              // the next problem refills LDS and the scratch
    }
}

constexpr int SPEC_SLICE = 16;                                        // settings per workgroup of kernel E2
constexpr int SPEC_EVAL_THREADS = 256;

// Kernel E2.  stats: the F * nsub packed blocks (category f nsub + s); galpha, grcond: the Q settings.  set[F + 1][Q][3],
// fit[Q][K] (problem F), coef[F][Q][K] (may be nullptr), held[F][Q][nsub][3].
__global__ __launch_bounds__(SPEC_EVAL_THREADS) void fsnap_spectral_eval_k(
    const double* __restrict__ stats, const double* __restrict__ folds, const double* __restrict__ total,
    const double* __restrict__ eig, const double* __restrict__ z, const double* __restrict__ V, const double* __restrict__ info,
    const double* __restrict__ galpha, const double* __restrict__ grcond, int K, int F, int nsub, int Q,
    double* __restrict__ set, double* __restrict__ fit, double* __restrict__ coef, double* __restrict__ held) {
    extern __shared__ __attribute__((aligned(16))) double spec_lds[];
    const int tid = threadIdx.x;
    const int KK = K * K;
    const int64_t T = (int64_t)KK + K + 3;
    double* lam = spec_lds;
    double* zz = lam + K;
    double* gg = zz + K;                                              // g[16][K]; later the rows of G beta
    double* bt = gg + SPEC_SLICE * K;                                 // beta[16][K]
    const int nslice = (Q + SPEC_SLICE - 1) / SPEC_SLICE;
    const int64_t nwork = (int64_t)(F + 1) * nslice;

    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int p = (int)(w / nslice), q0 = (int)(w - (int64_t)p * nslice) * SPEC_SLICE;
        const int nq = Q - q0 < SPEC_SLICE ? Q - q0 : SPEC_SLICE;
        const int n = (int)info[(int64_t)p * 6];
        const double lmax = info[(int64_t)p * 6 + 3];
        const FoldView fv = fold_view(folds, total, p, F, K);
        if (tid < K) {
            lam[tid] = eig[(int64_t)p * K + tid];
            zz[tid] = z[(int64_t)p * K + tid];
        }
        __syncthreads();
        for (int idx = tid; idx < nq * n; idx += SPEC_EVAL_THREADS) {
            const int q = idx / n, i = idx - q * n;
            gg[q * K + i] = spec_g(lam[i], zz[i], galpha[q0 + q], spec_cut(grcond[q0 + q], n, lmax));
        }
        if (tid < nq) {
            const SpecSet st = spec_setting(lam, zz, n, galpha[q0 + tid], spec_cut(grcond[q0 + tid], n, lmax), fv.y2);
            double* so = set + ((int64_t)p * Q + q0 + tid) * 3;
            so[0] = st.rank;
            so[1] = st.dof;
            so[2] = st.sse;
        }
        __syncthreads();
        if (tid < K) {                                                // beta_j of every setting of the slice, i ascending
            double acc[SPEC_SLICE];
#pragma unroll
            for (int q = 0; q < SPEC_SLICE; ++q) acc[q] = 0.0;
            const double* Vp = V + (int64_t)p * KK + tid;
            for (int i = 0; i < n; ++i) {
                const double v = Vp[(int64_t)i * K];
#pragma unroll
                for (int q = 0; q < SPEC_SLICE; ++q)
                    if (q < nq) acc[q] = fma(gg[q * K + i], v, acc[q]);
            }
#pragma unroll
            for (int q = 0; q < SPEC_SLICE; ++q)
                if (q < nq) {
                    bt[q * K + tid] = acc[q];
                    if (p == F)
                        fit[(int64_t)(q0 + q) * K + tid] = acc[q];
                    else if (coef)
                        coef[((int64_t)p * Q + q0 + q) * K + tid] = acc[q];
                }
        }
        __syncthreads();
        if (p < F) {
            for (int s = 0; s < nsub; ++s) {
                const double* blk = stats + ((int64_t)p * nsub + s) * T;
                if (tid < K) {                                        // row tid of G beta; G is symmetric: read down column tid
                    double acc[SPEC_SLICE];
#pragma unroll
                    for (int q = 0; q < SPEC_SLICE; ++q) acc[q] = 0.0;
                    for (int j = 0; j < K; ++j) {
                        const double gv = blk[(int64_t)j * K + tid];
#pragma unroll
                        for (int q = 0; q < SPEC_SLICE; ++q)
                            if (q < nq) acc[q] = fma(gv, bt[q * K + j], acc[q]);
                    }
#pragma unroll
                    for (int q = 0; q < SPEC_SLICE; ++q)
                        if (q < nq) gg[q * K + tid] = acc[q];
                }
                __syncthreads();
                if (tid < nq) {
                    double s1 = 0.0, s2 = 0.0;
                    for (int i = 0; i < K; ++i) {
                        const double b = bt[tid * K + i];
                        s1 = fma(b, blk[KK + i], s1);
                        s2 = fma(b, gg[tid * K + i], s2);
                    }
                    const double bb = blk[KK + K];
                    fold_heldout_store(held + (((int64_t)p * Q + q0 + tid) * nsub + s) * 3, blk[KK + K + 2], fma(-2.0, s1, bb) + s2, bb);
                }
                __syncthreads();                                      // gg is free for the next class
            }
        }
        __syncthreads();                                              // the next work item refills LDS
    }
}

}  // namespace

size_t spectral_eig_lds_bytes(int K) {
    return (spec_fixed_doubles(K) + (spec_vec_in_lds(K) ? (size_t)K * K : 0)) * 8 + spec_int_count(K) * 4;
}

bool spectral_vectors_in_lds(int K) { return spec_vec_in_lds(K); }

// One workgroup per CU whatever K: at 107 VGPRs a SIMD holds 4 waves, a CU 16, which is one workgroup of 1024 threads; the grid
// and the eigenvector scratch are sized for what can be resident.
int spectral_eig_blocks_per_cu(int) { return 1; }

size_t spectral_eval_lds_bytes(int K) { return (size_t)(2 + 2 * SPEC_SLICE) * K * 8; }

int spectral_eval_blocks_per_cu(int K) {
    const size_t per = (size_t)160 * 1024 / (spectral_eval_lds_bytes(K) + 512);
    return per < 1 ? 1 : per > 4 ? 4 : (int)per;
}

int spectral_slices(int Q) { return (Q + SPEC_SLICE - 1) / SPEC_SLICE; }

hipError_t launch_spectral_eig(int nblocks, const double* folds, const double* total, int K, int F, double* vwork, double* eig,
                               double* z, double* V, double* info, hipStream_t st) {
    if (K < 1 || K > SPEC_MAX_K || F < 1 || nblocks < 1) return hipErrorInvalidValue;
    // set on every launch: the attribute belongs to the current device, and the call costs microseconds next to the kernel
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_spectral_eig_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)SPEC_LDS_BUDGET);
    if (e != hipSuccess) return e;
    fsnap_spectral_eig_k<<<dim3((unsigned)nblocks), dim3(SPEC_THREADS), spectral_eig_lds_bytes(K), st>>>(
        folds, total, K, F, LOCO_PIVOT_TOL, vwork, eig, z, V, info);
    return hipGetLastError();
}

hipError_t launch_spectral_eval(int nblocks, const double* stats, const double* folds, const double* total, const double* eig,
                                const double* z, const double* V, const double* info, const double* alphas, const double* rconds,
                                int K, int F, int nsub, int Q, double* set, double* fit, double* coef, double* held,
                                hipStream_t st) {
    if (K < 1 || K > SPEC_MAX_K || F < 1 || nsub < 1 || Q < 1 || nblocks < 1) return hipErrorInvalidValue;
    fsnap_spectral_eval_k<<<dim3((unsigned)nblocks), dim3(SPEC_EVAL_THREADS), spectral_eval_lds_bytes(K), st>>>(
        stats, folds, total, eig, z, V, info, alphas, rconds, K, F, nsub, Q, set, fit, coef, held);
    return hipGetLastError();
}

}  // namespace fsnap
