// fsnap_robust.hip — the step between two fits of an M-estimator by iteratively re-weighted least squares (gfx950 only):
//   R0  fsnap_robust_pcat_k    class of every PARTICIPATING row (training row with w > 0), -1 for every other row; once per session
//   R1  fsnap_robust_rows_k    e_i = w_i (b_i - a_i . beta), one pass over A; optionally (scales known) the weights of R3 too
//   R2  fsnap_robust_hist_k / fsnap_robust_choose_k   exact per-class middle order statistics of |e| by radix selection
//   R3  fsnap_robust_rows_k without the rows (e read back): r_i, w_i r_i and the per-class sums from e, w and the scales
// Every sum is folded in a fixed order (per accumulating lane -> workgroup -> fsnap_colsum_partials_k); the only atomics are
// integer adds of the digit histograms, so every result is bit-identical from run to run.
#include "fsnap_device_common.h"
#include "fsnap_kernels.h"

// the weights are closed forms that the host yardstick (solvers/robust.py) evaluates operation by operation in fp64: no
// contraction of a * b + c into an fma outside the explicit __builtin_fma of the dot product
#pragma clang fp contract(off)

namespace fsnap {

namespace {

constexpr int ROBUST_NSUM = 6;     // per class: n, down-weighted, rejected, sum omega, sum e^2, sum rho
constexpr int ROBUST_SLOTS = 16;   // accumulating lanes of a workgroup: 4 waves x 4 row groups

__global__ __launch_bounds__(256) void fsnap_robust_pcat_k(const double* __restrict__ w, const unsigned char* __restrict__ mask,
                                                           const int* __restrict__ cat, int64_t m, int* __restrict__ pcat) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        const bool keep = (mask ? mask[i] != 0 : true) && w[i] > 0.0;           // NaN weights do not take part
        pcat[i] = keep ? (cat ? cat[i] : 0) : -1;
    }
}

// r = sqrt(omega) and rho of one residual: the closed forms of solvers/robust.py (robust_weight), same operations in the
// same order.  cs = c * s is the single fp64 product the branch is decided against; s == 0: r = 1, rho = 0.
__device__ __forceinline__ void robust_weight(int loss, double c, double s, double e, double& r, double& rho) {
    r = 1.0;
    rho = 0.0;
    if (!(s > 0.0)) return;
    const double cs = c * s, ae = fabs(e), u = e / s;
    if (loss == ROBUST_HUBER) {
        if (ae <= cs) {
            rho = (u * u) * 0.5;
        } else {
            r = sqrt(cs / ae);
            rho = c * fabs(u) - (c * c) * 0.5;
        }
    } else if (loss == ROBUST_BISQUARE) {
        const double c6 = (c * c) / 6.0;
        if (ae < cs) {
            const double t = e / cs;
            r = 1.0 - t * t;
            const double q = u / c, v = 1.0 - q * q;
            rho = c6 * (1.0 - (v * v) * v);
        } else {
            r = 0.0;
            rho = c6;
        }
    } else {
        const double t = e / cs;
        r = 1.0 / sqrt(1.0 + t * t);
        const double q = u / c;
        rho = ((c * c) * 0.5) * log(1.0 + q * q);
    }
}

template <int NJ>
struct RobustRows {
    d2u x[2][NJ > 0 ? NJ : 1];
};

// R1 / R3.  16 lanes per row, a wave takes 8 rows per step (two groups of four), waves stride over the rows; NJ > 0: the
// row (K <= 32 NJ columns) is fetched into registers by nontemporal 16-byte loads before the first use, NJ = 0: any width,
// a loop over the columns (the plan of kernel 4).  No load leaves the row: the last column of an odd-width row is read as
// the upper half of the pair before it (K = 1: a scalar load).  Rows that do not take part (pcat < 0) are zeroed by
// selects: NaN / Inf in them reach nothing.
//   e_in == nullptr: e_i from the rows, written to e_out;  e_in != nullptr: R3, e_i read back, A is not touched
//   do_weights: r_i -> r_out, w_i r_i -> wr_out, per-class sums -> partial[workgroup][ncat][6].  The sums are kept per
//   accumulating lane (lane 0 of a row group; slot = 4 wave + row group) in LDS and folded in slot order, so that a launch
//   with the rows and one without them add the same numbers in the same order whenever their grids agree.
template <int NJ>
__global__ __launch_bounds__(256) void fsnap_robust_rows_k(const double* __restrict__ A, int64_t lda,
                                                           const double* __restrict__ beta, int64_t m, int K,
                                                           const double* __restrict__ b, const double* __restrict__ w,
                                                           const int* __restrict__ pcat, const double* __restrict__ e_in,
                                                           double* __restrict__ e_out, int do_weights, int loss, double c,
                                                           const double* __restrict__ scale, double* __restrict__ r_out,
                                                           double* __restrict__ wr_out, double* __restrict__ partial, int ncat) {
    constexpr int KP = NJ > 0 ? NJ * 32 : 32;
    __shared__ __attribute__((aligned(16))) double sbeta[KP];
    extern __shared__ __attribute__((aligned(16))) double dyn[];       // NJ = 0: beta (K doubles, padded to even), then the sums
    const bool rows = e_in == nullptr;
    double* gbeta = dyn;
    double* sacc = dyn + ((NJ > 0 || !rows) ? 0 : ((K + 1) & ~1));
    if (rows) {
        if (NJ > 0) {
            for (int cc = threadIdx.x; cc < KP; cc += 256) sbeta[cc] = cc < K ? beta[cc] : 0.0;
        } else {
            for (int cc = threadIdx.x; cc < K; cc += 256) gbeta[cc] = beta[cc];
        }
    }
    const int nacc = do_weights ? ncat * ROBUST_NSUM * ROBUST_SLOTS : 0;
    for (int t = threadIdx.x; t < nacc; t += 256) sacc[t] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, e = lane & 15, kr = lane >> 4, wv = threadIdx.x >> 6;
    const int slot = wv * 4 + kr;
    constexpr int NJR = NJ > 0 ? NJ : 1;
    bool v1[NJR], v2[NJR], up[NJR];
    int coff[NJR];
    double be0[NJR], be1[NJR];
    if (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NJR; ++j) {
            const int cc = 2 * e + 32 * j;
            v1[j] = cc < K;
            v2[j] = cc + 1 < K;
            up[j] = v1[j] && !v2[j] && K >= 2;                  // last column of an odd width: upper half of the pair before it
            coff[j] = v2[j] ? cc : (up[j] ? cc - 1 : 0);        // lanes past the row's end re-read its first pair (selected away)
            be0[j] = sbeta[cc];
            be1[j] = sbeta[cc + 1];
        }
    }
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv, step = (int64_t)gridDim.x * 4 * 8;
    for (int64_t r0 = wave * 8; r0 < m; r0 += step) {
        double sd[2] = {0.0, 0.0};
        if (rows) {
            if (NJ > 0) {
                RobustRows<NJ> R;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int64_t row = r0 + 4 * h + kr;
                    const double* src = A + (row < m ? row : 0) * lda;
                    if (K == 1) {
                        R.x[h][0][0] = __builtin_nontemporal_load(src);
                        R.x[h][0][1] = 0.0;
                    } else {
#pragma unroll
                        for (int j = 0; j < NJR; ++j)
                            R.x[h][j] = __builtin_nontemporal_load(reinterpret_cast<const d2u*>(src + coff[j]));
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int64_t row = r0 + 4 * h + kr;
                    const bool keep = row < m && pcat[row < m ? row : 0] >= 0;
                    double s0 = 0.0, s1 = 0.0;
#pragma unroll
                    for (int j = 0; j < NJR; ++j) {
                        const double x0 = (keep && v1[j]) ? (up[j] ? R.x[h][j][1] : R.x[h][j][0]) : 0.0;
                        const double x1 = (keep && v2[j]) ? R.x[h][j][1] : 0.0;
                        s0 = __builtin_fma(x0, be0[j], s0);
                        s1 = __builtin_fma(x1, be1[j], s1);
                    }
                    sd[h] = s0 + s1;
                }
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int64_t row = r0 + 4 * h + kr;
                    const bool keep = row < m && pcat[row < m ? row : 0] >= 0;
                    const double* src = A + (row < m ? row : 0) * lda;
                    double s0 = 0.0, s1 = 0.0;
                    for (int cc = 2 * e; cc < K; cc += 32) {
                        const bool two = cc + 1 < K;
                        double x0, x1 = 0.0;
                        if (two) {
                            const d2u x = __builtin_nontemporal_load(reinterpret_cast<const d2u*>(src + cc));
                            x0 = x[0];
                            x1 = x[1];
                        } else {
                            x0 = __builtin_nontemporal_load(src + cc);
                        }
                        s0 = __builtin_fma(keep ? x0 : 0.0, gbeta[cc], s0);
                        s1 = __builtin_fma(keep ? x1 : 0.0, two ? gbeta[cc + 1] : 0.0, s1);
                    }
                    sd[h] = s0 + s1;
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                sd[h] += __shfl_xor(sd[h], 8, 64);
                sd[h] += __shfl_xor(sd[h], 4, 64);
                sd[h] += __shfl_xor(sd[h], 2, 64);
                sd[h] += __shfl_xor(sd[h], 1, 64);
            }
        }
        if (e == 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t row = r0 + 4 * h + kr;
                if (row >= m) continue;
                const int g = pcat[row];
                const bool keep = g >= 0;
                const double wi = w[row];
                double ev;
                if (rows) {
                    ev = keep ? wi * (b[row] - sd[h]) : 0.0;
                    e_out[row] = ev;
                } else {
                    ev = keep ? e_in[row] : 0.0;
                }
                if (do_weights) {
                    double r = 1.0, rho = 0.0;
                    if (keep) {
                        robust_weight(loss, c, scale[g], ev, r, rho);
                        double* a = sacc + (size_t)g * ROBUST_NSUM * ROBUST_SLOTS + slot;
                        a[0 * ROBUST_SLOTS] += 1.0;
                        a[1 * ROBUST_SLOTS] += r < 1.0 ? 1.0 : 0.0;
                        a[2 * ROBUST_SLOTS] += r == 0.0 ? 1.0 : 0.0;
                        a[3 * ROBUST_SLOTS] += r * r;
                        a[4 * ROBUST_SLOTS] += ev * ev;
                        a[5 * ROBUST_SLOTS] += rho;
                    }
                    r_out[row] = r;
                    wr_out[row] = keep ? wi * r : wi;
                }
            }
        }
    }
    if (do_weights) {
        __syncthreads();
        for (int t = threadIdx.x; t < ncat * ROBUST_NSUM; t += 256) {
            const double* a = sacc + (size_t)t * ROBUST_SLOTS;
            double s = 0.0;
            for (int k = 0; k < ROBUST_SLOTS; ++k) s += a[k];                  // slot order: fixed
            partial[(size_t)blockIdx.x * ncat * ROBUST_NSUM + t] = s;
        }
    }
}

// R2, one digit pass.  key = bit pattern of |e| (monotone for non-negative doubles, NaN above everything).  The two targets of
// a class (lower and upper middle order statistic) each carry the digits chosen so far in prefix[class][target]; a row adds 1
// to the bin of its digit of this pass in the histogram of every target whose prefix it still shares.  Histograms in LDS
// (ncat x 2 x 256 counters), then one integer atomic per non-empty bin into the global table.
__global__ __launch_bounds__(256) void fsnap_robust_hist_k(const double* __restrict__ e, const int* __restrict__ pcat, int64_t m,
                                                           const unsigned long long* __restrict__ prefix, int pass, int ncat,
                                                           unsigned int* __restrict__ table) {
    extern __shared__ unsigned int hist[];
    const int nbin = ncat * 2 * 256;
    for (int t = threadIdx.x; t < nbin; t += 256) hist[t] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        const int g = pcat[i];
        if (g < 0) continue;
        const unsigned long long key = (unsigned long long)__double_as_longlong(e[i]) & 0x7FFFFFFFFFFFFFFFull;
        const unsigned int digit = (unsigned int)(key >> shift) & 255u;
        const unsigned long long high = pass == 0 ? 0ull : key >> (shift + 8);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (pass == 0 || high == prefix[g * 2 + j]) atomicAdd(&hist[(g * 2 + j) * 256 + digit], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nbin; t += 256)
        if (hist[t]) atomicAdd(&table[t], hist[t]);
}

__global__ __launch_bounds__(256) void fsnap_robust_table_to_double_k(const unsigned int* __restrict__ table, int n,
                                                                      double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[t] = (double)table[t];
}

// R2, the choice of a digit: thread (class, target) walks its 256 bins (counts: the table, or its sum over the ranks as
// doubles), finds the bin that holds its rank, appends the digit to its prefix and clears its bins for the next pass.
// Pass 0 also derives n (all bins of a target) and the 0-based ranks (n - 1) / 2 and n / 2; after pass 7 the prefixes are
// the two order statistics themselves and scale = 1.4826 ((lo + hi) * 0.5) (0 for an empty class).
__global__ __launch_bounds__(64) void fsnap_robust_choose_k(unsigned int* __restrict__ table, const double* __restrict__ tsum,
                                                            int pass, int ncat, unsigned long long* __restrict__ prefix,
                                                            unsigned long long* __restrict__ rank, long long* __restrict__ count,
                                                            double* __restrict__ scale) {
    const int t = threadIdx.x;
    if (t < ncat * 2) {
        const int g = t >> 1, j = t & 1;
        unsigned int* bins = table + (size_t)t * 256;
        const double* dbins = tsum ? tsum + (size_t)t * 256 : nullptr;
        unsigned long long k = 0, pre = 0;
        if (pass == 0) {
            unsigned long long n = 0;
            for (int d = 0; d < 256; ++d) n += dbins ? (unsigned long long)dbins[d] : bins[d];
            if (j == 0) count[g] = (long long)n;
            k = n == 0 ? 0 : (j == 0 ? (n - 1) / 2 : n / 2);
            if (n == 0) k = ~0ull;        // empty class: no bin holds the rank, the prefix stays 0
        } else {
            k = rank[t];
            pre = prefix[t];
        }
        unsigned int digit = 0;
        if (k != ~0ull) {
            unsigned long long cum = 0;
            for (int d = 0; d < 256; ++d) {
                const unsigned long long cnt = dbins ? (unsigned long long)dbins[d] : bins[d];
                if (cum + cnt > k) {
                    digit = (unsigned int)d;
                    break;
                }
                cum += cnt;
            }
            k -= cum;
        }
        for (int d = 0; d < 256; ++d) bins[d] = 0u;
        pre = (pre << 8) | digit;
        prefix[t] = pre;
        rank[t] = k;
    }
    if (pass == 7) {
        __syncthreads();
        if (t < ncat) {
            const double lo = __longlong_as_double((long long)prefix[2 * t]), hi = __longlong_as_double((long long)prefix[2 * t + 1]);
            scale[t] = count[t] > 0 ? 1.4826 * ((lo + hi) * 0.5) : 0.0;
        }
    }
}

}  // namespace

int robust_num_blocks(int64_t m, int K) { return K <= 288 ? residual_num_blocks(m, K) : gemv_num_blocks(m); }

size_t robust_state_bytes(int ncat) {
    // prefix [ncat][2] | rank [ncat][2] | count [ncat] | scale [ncat] | table [ncat][2][256] u32 | table as doubles
    return (size_t)ncat * (16 + 16 + 8 + 8) + (size_t)ncat * 512 * 4 + (size_t)ncat * 512 * 8;
}

hipError_t launch_robust_pcat(const double* w, const unsigned char* mask, const int* cat, int64_t m, int* pcat, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    int64_t nb = (m + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(fsnap_robust_pcat_k, dim3((unsigned)nb), dim3(256), 0, st, w, mask, cat, m, pcat);
    return hipGetLastError();
}

hipError_t launch_robust_rows(const double* A, int64_t lda, const double* beta, int64_t m, int K, const double* b, const double* w,
                              const int* pcat, const double* e_in, double* e_out, bool do_weights, int loss, double c,
                              const double* scale, double* r_out, double* wr_out, double* partial, double* sums, int ncat,
                              hipStream_t st) {
    if (m <= 0 || K <= 0 || ncat < 1 || ncat > ROBUST_MAX_CLASSES) return hipErrorInvalidValue;
    const int nb = robust_num_blocks(m, K);
    const size_t accb = do_weights ? (size_t)ncat * ROBUST_NSUM * ROBUST_SLOTS * 8 : 0;
    const int nj = e_in ? 0 : (K + 31) / 32;
#define FSNAP_LAUNCH(NJ, LDS)                                                                                                    \
    hipLaunchKernelGGL((fsnap_robust_rows_k<NJ>), dim3((unsigned)nb), dim3(256), (LDS), st, A, lda, beta, m, K, b, w, pcat, e_in, \
                       e_out, do_weights ? 1 : 0, loss, c, scale, r_out, wr_out, partial, ncat)
    switch (nj) {
        case 1: FSNAP_LAUNCH(1, accb); break;
        case 2: FSNAP_LAUNCH(2, accb); break;
        case 3: FSNAP_LAUNCH(3, accb); break;
        case 4: FSNAP_LAUNCH(4, accb); break;
        case 5: FSNAP_LAUNCH(5, accb); break;
        case 6: FSNAP_LAUNCH(6, accb); break;
        case 7: case 8: FSNAP_LAUNCH(8, accb); break;
        case 9: FSNAP_LAUNCH(9, accb); break;
        default: {
            const size_t lds = accb + (e_in ? 0 : (size_t)((K + 1) & ~1) * 8);
            if (lds > 65536) return hipErrorInvalidValue;
            FSNAP_LAUNCH(0, lds);
        }
    }
#undef FSNAP_LAUNCH
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !do_weights) return err;
    return launch_colsum(partial, nb, ncat * ROBUST_NSUM, sums, st);
}

hipError_t launch_robust_hist(const double* e, const int* pcat, int64_t m, int pass, int ncat, void* state, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    char* p = (char*)state;
    const unsigned long long* prefix = (const unsigned long long*)p;
    unsigned int* table = (unsigned int*)(p + (size_t)ncat * 48);
    int64_t nb = (m + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(fsnap_robust_hist_k, dim3((unsigned)nb), dim3(256), (size_t)ncat * 512 * 4, st, e, pcat, m, prefix, pass,
                       ncat, table);
    return hipGetLastError();
}

double* robust_table_doubles(void* state, int ncat) { return (double*)((char*)state + (size_t)ncat * 48 + (size_t)ncat * 512 * 4); }
double* robust_scale_ptr(void* state, int ncat) { return (double*)((char*)state + (size_t)ncat * 40); }
long long* robust_count_ptr(void* state, int ncat) { return (long long*)((char*)state + (size_t)ncat * 32); }

hipError_t launch_robust_table_to_double(void* state, int ncat, hipStream_t st) {
    const unsigned int* table = (const unsigned int*)((char*)state + (size_t)ncat * 48);
    const int n = ncat * 512;
    hipLaunchKernelGGL(fsnap_robust_table_to_double_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, table, n,
                       robust_table_doubles(state, ncat));
    return hipGetLastError();
}

hipError_t launch_robust_choose(void* state, int pass, int ncat, bool summed, hipStream_t st) {
    char* p = (char*)state;
    hipLaunchKernelGGL(fsnap_robust_choose_k, dim3(1), dim3(64), 0, st, (unsigned int*)(p + (size_t)ncat * 48),
                       summed ? (const double*)robust_table_doubles(state, ncat) : (const double*)nullptr, pass, ncat,
                       (unsigned long long*)p, (unsigned long long*)(p + (size_t)ncat * 16), robust_count_ptr(state, ncat),
                       robust_scale_ptr(state, ncat));
    return hipGetLastError();
}

}  // namespace fsnap
