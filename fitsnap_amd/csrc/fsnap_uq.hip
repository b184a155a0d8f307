// fsnap_uq.hip — predictive variance of rows under a posterior covariance, one pass over the rows (gfx950 only).
//
// For every row a_i of A (m x K, leading dimension lda) and a small matrix M (K x J):
//   QUAD (J = K)  v_i = a_i^T M a_i        fullcov / loop (solver.py:440-472), (A C * A).sum(-1) of the AL loop
//   NORM          v_i = || a_i M ||^2      chol / choleye / svd / sam with M = L, shifted L, U sqrt(S), centred samples
// and optionally p_i = a_i . beta (the predictive mean) from the same read of the row.
//
//   U1  fsnap_uq_rows_k<NT, MODE>  K <= 144 (NT = ceil(K / 16) <= 9): a wave takes 2 blocks of 16 rows and keeps them in
//                                  registers for the whole pass (2 x 4 NT doubles per lane); T^T = M^T A_blk^T runs on
//                                  v_mfma_f64_16x16x4f64 one 16-column tile of M at a time: the A operand is the M tile
//                                  (lane (e, ks): M[4 s + ks][16 jt + e]), the B operand is the row block as it stands
//                                  (lane (e, ks): a_e[4 s + ks]), so D[reg g] at lane (e, ks) is T[e][16 jt + ks + 4 g].
//                                  The QUAD epilogue needs a_e[16 jt + ks + 4 g], a value of the same lane's row (re-read
//                                  from L1 / L2: keeping it in a register needs the tile loop unrolled, which spills).
//                                  The two row blocks share every M fragment (two independent accumulator chains).
//   U1G fsnap_uq_rows_gen_k<MODE>  K > 144 (untuned): the same tiles with the row values re-read (L1 / L2) per M tile
//   U2  fsnap_uq_chunk_k           per chunk of the category-sorted row index (fsnap_cat_chunks): sum and max of s_i v_i
//   U3  fsnap_uq_cat_k             per category: the chunks' sums in chunk order, their max
// T is never stored.  A row's result is a function of a_i, M, beta alone: its lane position within the block changes
// nothing (every D element is the same MFMA k-chain, the fold is per lane in a fixed order, then xor 16, xor 32), so results
// are bit-identical under any row subset, permutation, m or lda.  Category sums follow the stable-sorted row order.  No
// atomics; every result is written with vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_rowvar_body.h"

namespace {

constexpr int UQ_RB = fsnap_rowvar::RB;   // 16-row blocks per wave

template <int NT, int MODE>
__global__ __launch_bounds__(256, 2) void fsnap_uq_rows_k(const double* __restrict__ A, int64_t lda, int64_t m, int K,
                                                       const double* __restrict__ Mp, int Jp,
                                                       const double* __restrict__ bp, double* __restrict__ var,
                                                       double* __restrict__ preds) {
    constexpr int NS = 4 * NT;
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * UQ_RB);
    double x[UQ_RB][NS];
    int64_t row[UQ_RB];
    bool valid[UQ_RB];
#pragma unroll
    for (int r = 0; r < UQ_RB; ++r) {
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
    if (preds) {
#pragma unroll
        for (int r = 0; r < UQ_RB; ++r) {
            double p = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) p = __builtin_fma(x[r][s], bp[4 * s + ks], p);
            p = ks_sum(p);
            if (ks == 0 && valid[r]) preds[row[r]] = p;
        }
    }
    if (!var) return;
    double v[UQ_RB];
#pragma unroll
    for (int r = 0; r < UQ_RB; ++r) v[r] = 0.0;
    // one 16-column tile of M per step (a runtime loop: unrolling it over the tiles to keep the QUAD epilogue's row values
    // in registers spills at NT >= 8); the QUAD epilogue re-reads a_e[16 jt + ks + 4 g] (L1 / L2, the row was just read)
    const double* src[UQ_RB];
#pragma unroll
    for (int r = 0; r < UQ_RB; ++r) src[r] = A + (valid[r] ? row[r] : 0) * lda;
    const int njt = Jp / 16;
    for (int jt = 0; jt < njt; ++jt) {
        d4 acc[UQ_RB];
#pragma unroll
        for (int r = 0; r < UQ_RB; ++r) acc[r] = d4{0.0, 0.0, 0.0, 0.0};
        const double* mcol = Mp + 16 * jt + e;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double mf = mcol[(int64_t)(4 * s + ks) * Jp];
#pragma unroll
            for (int r = 0; r < UQ_RB; ++r) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(mf, x[r][s], acc[r], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < UQ_RB; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                double a = 0.0;
                if constexpr (MODE == fsnap::UQ_QUAD) {
                    const int k = 16 * jt + ks + 4 * g;
                    if (valid[r] && k < K) a = src[r][k];
                }
                v[r] = fsnap_rowvar::fold<MODE>(v[r], acc[r][g], a);     // NORM: padding columns of M are zero, they add nothing
            }
    }
#pragma unroll
    for (int r = 0; r < UQ_RB; ++r) {
        const double s = ks_sum(v[r]);
        if (ks == 0 && valid[r]) var[row[r]] = s;
    }
}

// Kernel U1G: any K (untuned).  Same lane mapping; the row values are loaded per k step of every M tile
// (fsnap_rowvar::rows_gen_body, shared with kernel B1G of fsnap_select.hip).
template <int MODE>
__global__ __launch_bounds__(256) void fsnap_uq_rows_gen_k(const double* __restrict__ A, int64_t lda, int64_t m, int K,
                                                           const double* __restrict__ Mp, int Jp,
                                                           const double* __restrict__ bp, double* __restrict__ var,
                                                           double* __restrict__ preds) {
    fsnap_rowvar::rows_gen_body<MODE, false>(A, lda, m, K, Mp, Jp, bp, var, preds);
}

// Kernel U2: one wave per chunk; lane l takes positions l, l + 64, ... of the chunk in order, then a fixed butterfly.
// part[chunk][2] = (sum, max) of s_i v_i over the chunk's rows (s = 1 without a scale).  (fsnap_rowvar::chunk_body, shared
// with kernel B2 of fsnap_select.hip.)
__global__ __launch_bounds__(64) void fsnap_uq_chunk_k(const double* __restrict__ var, const double* __restrict__ scale,
                                                       const int* __restrict__ idx, const fsnap::CatChunk* __restrict__ chunks,
                                                       double* __restrict__ part) {
    fsnap_rowvar::chunk_body(var, scale, idx, chunks, nullptr, part);
}

// Kernel U3: one thread per category, its chunks in order (cbeg[ncat + 1]); an empty category gets (0, -inf).
__global__ __launch_bounds__(256) void fsnap_uq_cat_k(const double* __restrict__ part, const int* __restrict__ cbeg, int ncat,
                                                     double* __restrict__ cat_sum, double* __restrict__ cat_max) {
    fsnap_rowvar::cat_body(part, cbeg, nullptr, ncat, cat_sum, cat_max);
}

}  // namespace

namespace fsnap {

hipError_t launch_uq_rows(int mode, const double* A, int64_t lda, int64_t m, int K, const double* Mp, int Jp, const double* bp,
                          double* var, double* preds, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    const int64_t rows_per_block = 4 * 16 * UQ_RB;
    const dim3 grid((unsigned)((m + rows_per_block - 1) / rows_per_block));
    auto launch = [&](auto nt, auto md) {
        constexpr int N = decltype(nt)::value, MODE = decltype(md)::value;
        if constexpr (N > 0) fsnap_uq_rows_k<N, MODE><<<grid, 256, 0, st>>>(A, lda, m, K, Mp, Jp, bp, var, preds);
        else fsnap_uq_rows_gen_k<MODE><<<grid, 256, 0, st>>>(A, lda, m, K, Mp, Jp, bp, var, preds);
    };
    dispatch_nt((K + 15) / 16, [&](auto nt) {
        if (mode == UQ_QUAD) launch(nt, std::integral_constant<int, UQ_QUAD>{});
        else launch(nt, std::integral_constant<int, UQ_NORM>{});
    });
    return hipGetLastError();
}

hipError_t launch_uq_cat(const double* var, const double* scale, const int* idx, const CatChunk* chunks, int64_t nchunks,
                         const int* cbeg, int ncat, double* part, double* cat_sum, double* cat_max, hipStream_t st) {
    if (nchunks > 0) fsnap_uq_chunk_k<<<dim3((unsigned)nchunks), 64, 0, st>>>(var, scale, idx, chunks, part);
    fsnap_uq_cat_k<<<dim3((unsigned)((ncat + 255) / 256)), 256, 0, st>>>(part, cbeg, ncat, cat_sum, cat_max);
    return hipGetLastError();
}

}  // namespace fsnap
