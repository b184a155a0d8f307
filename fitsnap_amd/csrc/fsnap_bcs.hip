// fsnap_bcs.hip — grouped K-fold BCS sparsity paths on the per-fold statistics (fsnap_bcs_path; the grid, the host route and the
// picks are solvers/bcs_path.py).  The BCS recurrence (fsnap_bcs_gram in fsnap_solve.cpp: the fast relevance-vector machine of
// Tipping & Faul as the reference's bcs() codes it) touches the rows only through (A^T A, A^T y, |y|^2, sum y, n), so with one
// packed block [G_f | c_f | bb_f, sum wb, n_f] per fold (fsnap_cat_normal_eq; summed by kernel S1 of fsnap_lasso.hip) the
// training system of fold f is "total minus block f" and the (F + 1) x Q problems (fold f left out, or none; setting q) are
// independent, strictly sequential recurrences on K x K systems with at most max_active <= 64 active columns.
//   Kernel B1: one workgroup of 256 threads (four waves) per problem, grid-stride.  Thread j owns column j (K <= 144): S_j,
//              Q_j, its position in the active set (-1: inactive) and its dead flag live in registers for the whole problem.
//              LDS holds Sig (max_active rows of the odd stride max_active | 1), the ACTIVE ROWS Qm[s_a, :] (max_active rows
//              of the odd stride K | 1, formed once as total row minus fold row when a column enters, so no iteration reads
//              the matrix from HBM again), mu, alpha and the column list by position and two work vectors: 108.5 KiB at
//              K = 144, max_active = 64, of the 160 KiB of a CU (one workgroup per CU there; more with a smaller max_active).
//              Per iteration: every thread scores its column (fsnap_bcs_body.h), two exact (ml, index) butterflies give the
//              best and the second-best column (the second for the margin), the chosen thread broadcasts its scalars through
//              LDS, then the re-estimate / add / delete update: thread a < n_active owns position a of mu and of the work
//              vectors, the n_active^2 entries of Sig are spread over the workgroup, and thread j walks down column j of the
//              active rows (consecutive lanes, consecutive addresses: conflict-free) for comm_j.
// fp64 VALU only, no atomics, plain vector stores.  Every sum runs in an order fixed by the problem alone (position ascending,
// one fma per term, the three sums of the noise estimate included; the held-out sums: the xor butterfly of fsnap_wave_sum.h) and
// the argmax takes the lowest index on equality: a problem's result is bit-identical run to run and under any permutation or
// subset of the grid or the folds.  The device's log may differ from the host's in the last bits, so results are not promised to
// be fsnap_bcs_gram's bits (on every case measured the fits were; the held-out sums are added in another order).
#include <hip/hip_runtime.h>

#include <cmath>

#include "fsnap_bcs_body.h"
#include "fsnap_fold_body.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap {
namespace {

constexpr int BCS_THREADS = 256;
constexpr int BCS_WAVES = BCS_THREADS / 64;
constexpr int BCS_NONE = 0x7FFFFFFF;           // the index of "no candidate"
constexpr int BCS_SIG_PER_THREAD = BCS_MAX_ACTIVE * BCS_MAX_ACTIVE / BCS_THREADS;   // 16

struct BcsLds {
    double* sig;      // Sig by position, stride lds
    double* rows;     // Qm[s_a, :] by position, stride ldr
    double* mu;       // by position
    double* al;       // alpha by position
    double* sigi;     // work: column p of Sig
    double* c1;       // work: comm1 of an addition; Q_ss mu at the end
    double* coef;     // dense coefficients (K)
    double* bc;       // 8 doubles the chosen thread broadcasts
    double* red;      // BCS_WAVES doubles of the block argmax
    int* idx;         // the active columns by position
    int* redi;        // BCS_WAVES ints of the block argmax
    int* bci;         // the chosen column's position
};

// argmax of (v, i) over the workgroup in numpy's order (bcs_before: a NaN wins, the lowest i on equality); (-inf, BCS_NONE)
// takes no part.  The same
// result in every thread.  Two barriers.
__device__ __forceinline__ void block_argmax(const BcsLds& s, double& v, int& i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (bcs_before(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    if (lane == 0) {
        s.red[wave] = v;
        s.redi[wave] = i;
    }
    __syncthreads();
    v = s.red[0];
    i = s.redi[0];
#pragma unroll
    for (int w = 1; w < BCS_WAVES; ++w) {
        const double ov = s.red[w];
        const int oi = s.redi[w];
        if (bcs_before(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    __syncthreads();                                                  // red is free again
}

// Kernel B1.  hyper[q][4] = sigma2 or 0, scale, eta, itermax.  P: the stride of a problem's pick list (>= every itermax).
__global__ __launch_bounds__(BCS_THREADS) void fsnap_bcs_path_k(const double* __restrict__ folds, const double* __restrict__ total,
                                                                const double* __restrict__ hyper, int K, int F, int Q, int MA,
                                                                int P, int exact, double pivot_tol, double* __restrict__ coef_out,
                                                                int* __restrict__ active_out, double* __restrict__ alpha_out,
                                                                double* __restrict__ errbar_out, int* __restrict__ picks_out,
                                                                double* __restrict__ info_out, double* __restrict__ heldout,
                                                                double* __restrict__ sig_out) {
    extern __shared__ __attribute__((aligned(16))) double bcs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KK = K * K, lds = MA | 1, ldr = K | 1;
    BcsLds s;
    s.sig = bcs_lds;
    s.rows = s.sig + MA * lds;
    s.mu = s.rows + MA * ldr;
    s.al = s.mu + MA;
    s.sigi = s.al + MA;
    s.c1 = s.sigi + MA;
    s.coef = s.c1 + MA;
    s.bc = s.coef + K;
    s.red = s.bc + 8;
    s.idx = (int*)(s.red + BCS_WAVES);
    s.redi = s.idx + MA;
    s.bci = s.redi + BCS_WAVES;
    const int nprob = (F + 1) * Q;
    const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const double nug = BCS_NUGGET;
    const bool own = tid < K;

    for (int p = blockIdx.x; p < nprob; p += gridDim.x) {
        const int f = p / Q, q = p - f * Q;
        const FoldView fv = fold_view(folds, total, f, F, K);
        const double* Gf = fv.Gf;
        const double y2 = fv.y2, n = fv.n;
        const double sum_y = Gf ? total[KK + K + 1] - Gf[KK + K + 1] : total[KK + K + 1];
        const double* hy = hyper + (int64_t)q * 4;
        const double s2 = hy[0] > 0.0 ? hy[0] : bcs_sigma2(hy[1], y2, sum_y, n);
        const double eta = hy[2];
        const int itermax = (int)hy[3];
        auto qm = [&](int r, int c) {
            const int64_t at = (int64_t)r * K + c;
            return Gf ? total[at] - Gf[at] : total[at];
        };
        int* picks = picks_out + (int64_t)p * P * 2;
        for (int e = tid; e < 2 * P; e += BCS_THREADS) picks[e] = -1;

        // the columns: dead flags, the diagonal and the right-hand side in registers
        double qjj = 0.0, qj = 0.0, Sj = 0.0, Qj = 0.0;
        bool dead = true;
        int pos = -1;
        if (own) {
            const double tjj = total[(int64_t)tid * K + tid];
            qjj = qm(tid, tid);
            dead = fold_dead(tjj, qjj, pivot_tol);
            qj = Gf ? total[KK + tid] - Gf[KK + tid] : total[KK + tid];
            s.coef[tid] = 0.0;
        }
        double br = own && !dead ? bcs_ratio(qj, qjj) : -inf;
        int i0 = own && !dead ? tid : BCS_NONE;
        block_argmax(s, br, i0);

        int na = 0, iters = 0, status = 0;
        double margin = inf;
        if (i0 != BCS_NONE) {
            if (tid == i0) {
                s.bc[0] = qjj;
                s.bc[1] = qj;
            }
            if (own) s.rows[tid] = qm(i0, tid);
            __syncthreads();
            const double Qii = s.bc[0], qi = s.bc[1];
            const double alpha0 = Qii / (br - s2);
            const double Sg00 = 1.0 / ((alpha0 + Qii / s2) + nug);
            if (own && !dead) {
                const double left = s.rows[tid] / s2;
                Sj = qjj / s2 - Sg00 * (left * left);
                Qj = qj / s2 - ((Sg00 * qi) / s2) * left;
            }
            if (tid == i0) pos = 0;
            __syncthreads();                                          // bc is read
            if (tid == 0) {
                s.sig[0] = Sg00;
                s.mu[0] = Sg00 * qi / s2;
                s.al[0] = alpha0;
                s.idx[0] = i0;
            }
            na = 1;
            __syncthreads();
            double ml0 = 0.0, mlprev = 0.0;
            status = 2;
            for (int count = 0; count < itermax; ++count) {
                BcsScore sc;
                sc.ml = -inf;
                sc.theta = 0.0;
                sc.ss = 0.0;
                if (own && !dead) sc = bcs_score(Sj, Qj, pos >= 0, pos >= 0 ? s.al[pos] : 0.0, na < MA);
                double mlb = sc.ml;
                int ib = sc.ml != -inf ? tid : BCS_NONE;
                block_argmax(s, mlb, ib);
                if (ib == BCS_NONE) {                                 // a guard: see fsnap_bcs_gram
                    status = 0;
                    break;
                }
                double ml2 = tid == ib ? -inf : sc.ml;
                int i2 = (tid != ib && sc.ml != -inf) ? tid : BCS_NONE;
                block_argmax(s, ml2, i2);
                if (i2 != BCS_NONE) {
                    const double m = (mlb - ml2) / fabs(mlb);
                    if (m < margin) margin = m;
                }
                iters = count + 1;
                if (count == 0) ml0 = mlb;
                const bool stop = count > 1 && fabs(mlb - mlprev) < fabs(mlb - ml0) * eta;
                mlprev = mlb;
                if (stop) {
                    if (tid == 0) {
                        picks[2 * count] = ib;
                        picks[2 * count + 1] = BCS_STOP;
                    }
                    status = 0;
                    break;
                }
                if (tid == ib) {
                    s.bc[0] = sc.theta;
                    s.bc[1] = sc.ss;
                    s.bc[2] = Sj;
                    s.bc[3] = Qj;
                    s.bc[4] = pos >= 0 ? s.al[pos] : 0.0;
                    s.bc[5] = pos >= 0 ? s.mu[pos] : 0.0;
                    s.bc[6] = pos >= 0 ? s.sig[pos * lds + pos] : 0.0;
                    s.bci[0] = pos;
                }
                __syncthreads();
                const double th = s.bc[0], ssb = s.bc[1], Sb = s.bc[2], Qb = s.bc[3], alb = s.bc[4], mub = s.bc[5], sgb = s.bc[6];
                const int pb = s.bci[0];
                int action;
                bool last = false;
                if (th > 0.0) {
                    const double a_new = ssb * ssb / th + nug;
                    if (pb >= 0) {                                    // re-estimate
                        action = BCS_RE;
                        if (tid < na) s.sigi[tid] = s.sig[tid * lds + pb];
                        __syncthreads();
                        const double delta = a_new - alb;
                        const double ki = delta / (1.0 + sgb * delta);
                        if (tid < na) s.mu[tid] -= (ki * mub) * s.sigi[tid];
                        for (int e = tid; e < na * na; e += BCS_THREADS) {
                            const int a = e / na, b = e - a * na;
                            s.sig[a * lds + b] -= ki * (s.sigi[a] * s.sigi[b]);
                        }
                        if (own && !dead) {
                            double c = 0.0;
                            for (int a = 0; a < na; ++a) c = fma(s.rows[a * ldr + tid], s.sigi[a], c);
                            c /= s2;
                            Sj += ki * (c * c);
                            Qj += (ki * mub) * c;
                        }
                        if (tid == 0) s.al[pb] = a_new;
                    } else {                                          // add
                        action = BCS_ADD;
                        const double Sigii = 1.0 / (a_new + Sb);
                        const double mui = Sigii * Qb;
                        if (own) s.rows[na * ldr + tid] = qm(ib, tid);
                        __syncthreads();
                        if (tid < na) {
                            double t = 0.0;
                            for (int b = 0; b < na; ++b) t = fma(s.sig[tid * lds + b], s.rows[b * ldr + ib], t);
                            s.c1[tid] = t / s2;
                        }
                        __syncthreads();
                        if (own && !dead) {
                            double c = 0.0;
                            for (int a = 0; a < na; ++a) c = fma(s.rows[a * ldr + tid], s.c1[a], c);
                            const double c2 = (s.rows[na * ldr + tid] - c) / s2;
                            Sj -= Sigii * (c2 * c2);
                            Qj -= mui * c2;
                        }
                        for (int e = tid; e < na * na; e += BCS_THREADS) {
                            const int a = e / na, b = e - a * na;
                            s.sig[a * lds + b] += Sigii * (s.c1[a] * s.c1[b]);
                        }
                        if (tid < na) {
                            const double off = -Sigii * s.c1[tid];
                            s.sig[tid * lds + na] = off;
                            s.sig[na * lds + tid] = off;
                            s.mu[tid] -= mui * s.c1[tid];
                        }
                        if (tid == 0) {
                            s.sig[na * lds + na] = Sigii;
                            s.mu[na] = mui;
                            s.al[na] = a_new;
                            s.idx[na] = ib;
                        }
                        if (tid == ib) pos = na;
                        ++na;
                    }
                } else if (pb < 0) {                                  // an inactive column without theta > 0 (its ml is NaN): the
                    action = BCS_STOP;                                // reference idles on this state until itermax
                    last = true;
                } else {                                              // delete
                    if (na > 1) {
                        action = BCS_DEL;
                        if (tid < na) s.sigi[tid] = s.sig[tid * lds + pb];
                        __syncthreads();
                        for (int e = tid; e < na * na; e += BCS_THREADS) {
                            const int a = e / na, b = e - a * na;
                            s.sig[a * lds + b] -= (s.sigi[a] * s.sigi[b]) / sgb;
                        }
                        if (exact) {
                            if (tid < na) s.mu[tid] -= (mub / sgb) * s.sigi[tid];
                            if (own && !dead) {
                                double c = 0.0;
                                for (int a = 0; a < na; ++a) c = fma(s.rows[a * ldr + tid], s.sigi[a], c);
                                c /= s2;
                                Sj += (c * c) / sgb;
                                Qj += (mub / sgb) * c;
                            }
                        }
                        __syncthreads();
                        // compact: position pb leaves.  Every thread reads what it will write, then all write.
                        const int nn = na - 1;
                        double keep[BCS_SIG_PER_THREAD];
#pragma unroll
                        for (int u = 0; u < BCS_SIG_PER_THREAD; ++u) {
                            const int e = tid + u * BCS_THREADS;
                            keep[u] = 0.0;
                            if (e < nn * nn) {
                                const int a = e / nn, b = e - a * nn;
                                keep[u] = s.sig[(a + (a >= pb ? 1 : 0)) * lds + b + (b >= pb ? 1 : 0)];
                            }
                        }
                        double kmu = 0.0, kal = 0.0;
                        int kidx = 0;
                        if (tid < nn) {
                            const int o = tid + (tid >= pb ? 1 : 0);
                            kmu = s.mu[o];
                            kal = s.al[o];
                            kidx = s.idx[o];
                        }
                        __syncthreads();
#pragma unroll
                        for (int u = 0; u < BCS_SIG_PER_THREAD; ++u) {
                            const int e = tid + u * BCS_THREADS;
                            if (e < nn * nn) {
                                const int a = e / nn, b = e - a * nn;
                                s.sig[a * lds + b] = keep[u];
                            }
                        }
                        if (tid < nn) {
                            s.mu[tid] = kmu;
                            s.al[tid] = kal;
                            s.idx[tid] = kidx;
                        }
                        if (own)                                      // thread j moves its own column of the rows up
                            for (int a = pb; a < nn; ++a) s.rows[a * ldr + tid] = s.rows[(a + 1) * ldr + tid];
                        if (pos == pb)
                            pos = -1;
                        else if (pos > pb)
                            --pos;
                        na = nn;
                    } else {
                        action = BCS_STOP;
                    }
                    last = na == 1;
                }
                if (tid == 0) {
                    picks[2 * count] = ib;
                    picks[2 * count + 1] = action;
                }
                __syncthreads();                                      // the state of the next iteration is in place
                if (last) {
                    status = 0;
                    break;
                }
            }
        }
        // the fit, the re-estimated noise variance, the outputs by position
        __syncthreads();
        if (tid < na) {
            double t = 0.0;
            for (int b = 0; b < na; ++b) t = fma(s.rows[tid * ldr + s.idx[b]], s.mu[b], t);
            s.c1[tid] = t;
            s.coef[s.idx[tid]] = s.mu[tid];
            const int j = s.idx[tid];
            s.sigi[tid] = Gf ? total[KK + j] - Gf[KK + j] : total[KK + j];
        }
        __syncthreads();
        // the three sums of the noise estimate, in every thread and in fsnap_bcs_gram's order (position ascending, one fma per
        // term): identical bits in every thread, and the host route's bits
        double mq = 0.0, mQm = 0.0, ad = 0.0;
        for (int a = 0; a < na; ++a) {
            mq = fma(s.mu[a], s.sigi[a], mq);
            mQm = fma(s.mu[a], s.c1[a], mQm);
            ad = fma(s.al[a], s.sig[a * lds + a], ad);
        }
        const double rss = fma(-2.0, mq, y2) + mQm;
        const double s2_new = rss / (n - (double)na + ad);
        bool bad = false;
        {
            const int64_t at = (int64_t)p * MA;
            for (int a = tid; a < MA; a += BCS_THREADS) {
                const double d = a < na ? s.sig[a * lds + a] : 0.0;
                const double eb = sqrt(d < 0.0 ? 0.0 : d);
                const double m = a < na ? s.mu[a] : 0.0;
                bad = bad || !isfinite(eb) || !isfinite(m);
                active_out[at + a] = a < na ? s.idx[a] : -1;
                alpha_out[at + a] = a < na ? s.al[a] : 0.0;
                errbar_out[at + a] = eb;
            }
        }
        if (f == F) {
            double* so = sig_out + (int64_t)q * MA * MA;
            for (int e = tid; e < MA * MA; e += BCS_THREADS) {
                const int a = e / MA, b = e - a * MA;
                so[e] = (a < na && b < na) ? s.sig[a * lds + b] : 0.0;
            }
        }
        bad = __syncthreads_or(bad ? 1 : 0) != 0;
        // det(Sig) > -nugget by symmetric elimination without pivoting, in place: Sig is not needed any more
        double det = 1.0;
        for (int k = 0; k < na; ++k) {
            const double piv = s.sig[k * lds + k];
            det *= piv;
            const int r = na - k - 1;
            for (int e = tid; e < r * r; e += BCS_THREADS) {
                const int a = k + 1 + e / r, b = k + 1 + e % r;
                s.sig[a * lds + b] -= s.sig[a * lds + k] * s.sig[k * lds + b] / piv;
            }
            __syncthreads();
        }
        if (bad || !(det > -nug)) status = 1;
        if (own) {
            if (status == 1) s.coef[tid] = nan;
            coef_out[(int64_t)p * K + tid] = s.coef[tid];
        }
        if (tid == 0) {
            double* io = info_out + (int64_t)p * 6;
            io[0] = (double)iters;
            io[1] = (double)status;
            io[2] = s2;
            io[3] = s2_new;
            io[4] = rss;
            io[5] = margin;
        }
        __syncthreads();
        if (Gf) {
            // weighted squared error of fold f under its own refit, from the fold's statistics: bb_f - 2 beta . c_f + beta^T G_f beta
            // (sigi and c1 hold at most max_active entries, so the K row results go through the first row of the active rows)
            double* rv = s.rows;
            for (int i = wave; i < K; i += BCS_WAVES) {
                const double* row = Gf + (int64_t)i * K;
                double acc = 0.0;
                for (int j = lane; j < K; j += 64) acc += row[j] * s.coef[j];
                acc = wave_sum(acc);
                if (lane == 0) rv[i] = acc;
            }
            __syncthreads();
            if (wave == 0) {
                double s1 = 0.0, s2h = 0.0;
                for (int e = lane; e < K; e += 64) {
                    s1 += s.coef[e] * Gf[KK + e];
                    s2h += s.coef[e] * rv[e];
                }
                s1 = wave_sum(s1);
                s2h = wave_sum(s2h);
                // p = f Q + q for f < F
                if (lane == 0) fold_heldout_store(heldout + (int64_t)p * 3, fv.n_f, fv.bb_f - 2.0 * s1 + s2h, fv.bb_f);
            }
        }
        __syncthreads();                                              // the next problem refills LDS
    }
}

}  // namespace

size_t bcs_lds_bytes(int K, int max_active) {
    const size_t MA = (size_t)max_active;
    return (MA * (MA | 1) + MA * ((size_t)K | 1) + 4 * MA + (size_t)K + 8 + BCS_WAVES) * 8 + (MA + BCS_WAVES + 2) * 4;
}

int bcs_blocks_per_cu(int K, int max_active) {
    const size_t per = (size_t)160 * 1024 / (bcs_lds_bytes(K, max_active) + 512);
    return per < 1 ? 1 : per > 4 ? 4 : (int)per;
}

hipError_t launch_bcs_path(int nblocks, const double* folds, const double* total, const double* hyper, int K, int F, int Q,
                           int max_active, int P, int exact, double* coef, int* active, double* alpha, double* errbars, int* picks,
                           double* info, double* heldout, double* sig, hipStream_t st) {
    if (K < 1 || K > BCS_MAX_K || max_active < 1 || max_active > BCS_MAX_ACTIVE || max_active > K || P < 1 || nblocks < 1)
        return hipErrorInvalidValue;
    // set on every launch: the attribute belongs to the current device, and the call costs microseconds next to the kernel
    hipError_t e = hipFuncSetAttribute((const void*)fsnap_bcs_path_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bcs_lds_bytes(BCS_MAX_K, BCS_MAX_ACTIVE));
    if (e != hipSuccess) return e;
    fsnap_bcs_path_k<<<dim3((unsigned)nblocks), dim3(BCS_THREADS), bcs_lds_bytes(K, max_active), st>>>(
        folds, total, hyper, K, F, Q, max_active, P, exact, LOCO_PIVOT_TOL, coef, active, alpha, errbars, picks, info, heldout, sig);
    return hipGetLastError();
}

}  // namespace fsnap
