// fsnap_select.hip — greedy batch selection: downdate of resident per-row variances and the pick of a category (gfx950 only).
//
// The posterior covariance after a picked unit is C - V V^T (V: K x J, solvers/select.py), so the variance of every row
// drops by || a_i V ||^2.  The variances stay on the device between picks; a pick brings one (category, score) pair back.
//
//   B1  fsnap_sel_rows_k<NT>   K <= 144 (NT = ceil(K / 16) <= 9): var[i] -= || a_i V ||^2.  The register plan of U1 in NORM form
//                              (fsnap_uq.hip): a wave takes 2 blocks of 16 rows and keeps them in registers (2 x 4 NT doubles
//                              per lane), T^T = V^T A_blk^T on v_mfma_f64_16x16x4f64 one 16-column tile of V at a time (its
//                              fragments prefetched 7 ... 12 deep, across tiles), fold t^2 per lane, xor 16, xor 32, then ONE
//                              subtraction from the row's old variance.
//   B1G fsnap_sel_rows_gen_k   K > 144 (untuned): U1G's body (fsnap_rowvar_body.h) with the subtraction at its end
//   B2  fsnap_sel_chunk_k      U2's body: per chunk of the category-sorted row index sum and max of s_i var_i -- chunks of
//                              retired categories are skipped
//   B3  fsnap_sel_cat_k        U3's body: per live category the chunks' sums in chunk order, their max
//   B4  fsnap_sel_pick_k       one workgroup: arg-max of the objective (sum, max, sum / count) over the live categories, ties
//                              to the lowest id; writes (score, category) and, when asked, retires the category
// The subtracted value is bit for bit what U1 / U1G give in NORM mode for the same (a_i, V): a row's new variance depends on
// a_i, its old variance and V alone -- bit-identical run to run and under any row subset, permutation, m or lda.  Category
// sums follow the stable-sorted row order.  No atomics; every result is written with vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_rowvar_body.h"

namespace {

constexpr int SEL_RB = fsnap_rowvar::RB;   // 16-row blocks per wave

// fragments of V in flight: a divisor of NS (the slot of fragment s is s % PF in every tile), 7 ... 12 where there is one
constexpr int sel_prefetch_depth(int ns) {
    for (int d : {8, 9, 10, 7, 12, 6, 5, 4})
        if (d <= ns && ns % d == 0) return d;
    return 1;
}

template <int NT>
__global__ __launch_bounds__(256, 2) void fsnap_sel_rows_k(const double* __restrict__ A, int64_t lda, int64_t m, int K,
                                                        const double* __restrict__ Vp, int Jp, double* __restrict__ var) {
    constexpr int NS = 4 * NT;
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * SEL_RB);
    double x[SEL_RB][NS];
    int64_t row[SEL_RB];
    bool valid[SEL_RB];
#pragma unroll
    for (int r = 0; r < SEL_RB; ++r) {
        row[r] = row0 + 16 * r + e;
        valid[r] = row[r] < m;
        const double* src = A + (valid[r] ? row[r] : 0) * lda;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = 4 * s + ks;
            double v = 0.0;
            if (valid[r] && k < K) v = src[k];
            x[r][s] = v;
        }
    }
    double v[SEL_RB];
#pragma unroll
    for (int r = 0; r < SEL_RB; ++r) v[r] = 0.0;
    // the V fragments of a lane, (4 s + ks, 16 jt + e) for s = 0 ... NS - 1 and jt = 0 ... njt - 1, are one stream: PF of them
    // are kept in flight in a rotating set of registers, across the tile boundary too (the last tile re-reads itself)
    constexpr int PF = sel_prefetch_depth(NS);
    const int njt = Jp / 16;
    const double* vlane = Vp + (int64_t)ks * Jp + e;
    double vf[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) vf[i] = vlane[(int64_t)(4 * i) * Jp];
    for (int jt = 0; jt < njt; ++jt) {
        d4 acc[SEL_RB];
#pragma unroll
        for (int r = 0; r < SEL_RB; ++r) acc[r] = d4{0.0, 0.0, 0.0, 0.0};
        const double* vcol = vlane + 16 * jt;
        const double* vnext = vlane + 16 * (jt + 1 < njt ? jt + 1 : jt);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double cur = vf[s % PF];
            vf[s % PF] = s + PF < NS ? vcol[(int64_t)(4 * (s + PF)) * Jp] : vnext[(int64_t)(4 * (s + PF - NS)) * Jp];
#pragma unroll
            for (int r = 0; r < SEL_RB; ++r) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur, x[r][s], acc[r], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < SEL_RB; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) v[r] = __builtin_fma(acc[r][g], acc[r][g], v[r]);   // padding columns of V are zero
    }
#pragma unroll
    for (int r = 0; r < SEL_RB; ++r) {
        const double s = ks_sum(v[r]);
        if (ks == 0 && valid[r]) var[row[r]] = var[row[r]] - s;
    }
}

// Kernel B1G: any K (untuned): the body of U1G in NORM form with the subtraction in place of the store.
__global__ __launch_bounds__(256) void fsnap_sel_rows_gen_k(const double* __restrict__ A, int64_t lda, int64_t m, int K,
                                                            const double* __restrict__ Vp, int Jp, double* __restrict__ var) {
    fsnap_rowvar::rows_gen_body<fsnap::UQ_NORM, true>(A, lda, m, K, Vp, Jp, nullptr, var, nullptr);
}

// Kernel B2: the body of U2; a chunk of a retired category keeps what it had.
__global__ __launch_bounds__(64) void fsnap_sel_chunk_k(const double* __restrict__ var, const double* __restrict__ scale,
                                                        const int* __restrict__ idx, const fsnap::CatChunk* __restrict__ chunks,
                                                        const int* __restrict__ alive, double* __restrict__ part) {
    fsnap_rowvar::chunk_body(var, scale, idx, chunks, alive, part);
}

// Kernel B3: the body of U3 over the live categories.
__global__ __launch_bounds__(256) void fsnap_sel_cat_k(const double* __restrict__ part, const int* __restrict__ cbeg,
                                                      const int* __restrict__ alive, int ncat, double* __restrict__ cat_sum,
                                                      double* __restrict__ cat_max) {
    fsnap_rowvar::cat_body(part, cbeg, alive, ncat, cat_sum, cat_max);
}

// (a, ca) is better than (b, cb): larger key, ties to the lower id; id -1 = nothing yet.  A NaN score ranks as -inf.
__device__ __forceinline__ bool sel_better(double a, int ca, double b, int cb) {
    if (ca < 0) return false;
    if (cb < 0) return true;
    const double ka = a == a ? a : -__builtin_inf(), kb = b == b ? b : -__builtin_inf();
    return ka > kb || (ka == kb && ca < cb);
}

// Kernel B4: one workgroup of 1024 threads.  out[0] = score, out[1] = the category as a double (-1: none alive).
constexpr int SEL_PICK_THREADS = 1024;
__global__ __launch_bounds__(SEL_PICK_THREADS) void fsnap_sel_pick_k(const double* __restrict__ cat_sum,
                                                                   const double* __restrict__ cat_max,
                                                                   const int64_t* __restrict__ count, int* __restrict__ alive,
                                                                   int ncat, int objective, int retire, double* __restrict__ out) {
    __shared__ double ss[SEL_PICK_THREADS];
    __shared__ int sc[SEL_PICK_THREADS];
    const int t = threadIdx.x;
    double best = 0.0;
    int bc = -1;
    for (int c = t; c < ncat; c += SEL_PICK_THREADS) {
        if (!alive[c]) continue;
        double s;
        if (objective == fsnap::SEL_MAX) s = cat_max[c];
        else if (objective == fsnap::SEL_MEAN) s = cat_sum[c] / (double)count[c];
        else s = cat_sum[c];
        if (sel_better(s, c, best, bc)) {
            best = s;
            bc = c;
        }
    }
    ss[t] = best;
    sc[t] = bc;
    __syncthreads();
    for (int o = SEL_PICK_THREADS / 2; o > 0; o >>= 1) {
        if (t < o && sel_better(ss[t + o], sc[t + o], ss[t], sc[t])) {
            ss[t] = ss[t + o];
            sc[t] = sc[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = sc[0] >= 0 ? ss[0] : 0.0;
        out[1] = (double)sc[0];
        if (retire && sc[0] >= 0) alive[sc[0]] = 0;
    }
}

}  // namespace

namespace fsnap {

hipError_t launch_sel_rows(const double* A, int64_t lda, int64_t m, int K, const double* Vp, int Jp, double* var,
                           hipStream_t st) {
    if (m <= 0) return hipSuccess;
    const int64_t rows_per_block = 4 * 16 * SEL_RB;
    const dim3 grid((unsigned)((m + rows_per_block - 1) / rows_per_block));
    dispatch_nt((K + 15) / 16, [&](auto nt) {
        constexpr int N = decltype(nt)::value;
        if constexpr (N > 0) fsnap_sel_rows_k<N><<<grid, 256, 0, st>>>(A, lda, m, K, Vp, Jp, var);
        else fsnap_sel_rows_gen_k<<<grid, 256, 0, st>>>(A, lda, m, K, Vp, Jp, var);
    });
    return hipGetLastError();
}

hipError_t launch_sel_scores(const double* var, const double* scale, const int* idx, const CatChunk* chunks, int64_t nchunks,
                             const int* cbeg, const int* alive, int ncat, double* part, double* cat_sum, double* cat_max,
                             hipStream_t st) {
    if (nchunks > 0) fsnap_sel_chunk_k<<<dim3((unsigned)nchunks), 64, 0, st>>>(var, scale, idx, chunks, alive, part);
    fsnap_sel_cat_k<<<dim3((unsigned)((ncat + 255) / 256)), 256, 0, st>>>(part, cbeg, alive, ncat, cat_sum, cat_max);
    return hipGetLastError();
}

hipError_t launch_sel_pick(const double* cat_sum, const double* cat_max, const int64_t* count, int* alive, int ncat,
                           int objective, int retire, double* out, hipStream_t st) {
    fsnap_sel_pick_k<<<1, SEL_PICK_THREADS, 0, st>>>(cat_sum, cat_max, count, alive, ncat, objective, retire, out);
    return hipGetLastError();
}

}  // namespace fsnap
