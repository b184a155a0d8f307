// fsnap_mcmc.hip — weighted residual sums of up to 16 coefficient vectors in one pass over the resident rows (gfx950 only).
//
// For P <= 16 vectors u_p (K columns) and the rows of the current mask (weight zero included):
//     sse[p] = sum_i (w_i (a_i . u_p - b_i))^2        n = number of rows in the mask
// This is the log-posterior of the reference's MCMC solver (mcmc.py:80-88 logpost) up to constants, for the proposals of
// a speculated reject chain (solvers/mcmc.py).
//
//   S1  fsnap_sse_rows_k<NT>  K <= 144 (NT = ceil(K / 16) <= 9): a wave takes 16-row blocks in a grid-stride loop; the block
//                             is loaded into registers (lane (e, ks) holds row e's columns 16 j + 4 ks ... + 3 of every
//                             16-column chunk j, one 32-byte load per chunk) and multiplied on v_mfma_f64_16x16x4f64 with
//                             the U tile as the A operand (lane (p, ks) at step s = 4 j + t: U[p][16 j + 4 ks + t], from LDS)
//                             and the row block as the B operand, so D[reg g] at lane (e, ks) is a_e . u_{ks + 4 g}.
//   S1G fsnap_sse_rows_k<0>   K >  144 (untuned): the same tiles, the chunks of a row loaded and consumed one at a time, U
//                             read from global memory (L1 / L2) at every step
// Epilogue per lane: r = w_e (d - b_e), acc[g] += r^2 for rows of the mask, in block order; then the 16 rows of a lane group
// (xor 8, 4, 2, 1), the four waves through LDS, and one partial row [sse_0 .. sse_15 | n] per workgroup, folded in a fixed
// order by fsnap_colsum_partials_k.  Every slot goes through the same MFMA k-chain, the same per-lane order and the same fold
// tree, and the number of workgroups depends on m alone, so sse[p] depends on u_p and the rows only: bit-identical in any
// slot, for any P, whatever the other vectors are, and run to run.  Rows that do not take part (test rows, the padding rows
// of a ragged last block) are dropped by selects: NaN / Inf in them reach nothing.  No atomics; results are written with
// vector stores.
#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"

namespace {

typedef double d4u __attribute__((ext_vector_type(4), aligned(8)));

constexpr int SSE_NCOL = fsnap::SSE_MAX_P + 1;   // [sse_0 .. sse_15 | n]

// columns 16 j + 4 ks ... + 3 of a row, zero past K
__device__ __forceinline__ d4u sse_chunk(const double* src, int c0, int K) {
    if (c0 + 4 <= K) return *reinterpret_cast<const d4u*>(src + c0);
    d4u x;
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = c0 + t < K ? src[c0 + t] : 0.0;
    return x;
}

template <int NT>
__global__ __launch_bounds__(256) void fsnap_sse_rows_k(const double* __restrict__ A, int64_t lda, int64_t m, int K,
                                                        const double* __restrict__ Up, const double* __restrict__ b,
                                                        const double* __restrict__ w, const unsigned char* __restrict__ mask,
                                                        double* __restrict__ partial) {
    constexpr int NS = NT > 0 ? 4 * NT : 1;
    __shared__ double sU[NS * 64];
    __shared__ double fold[4][SSE_NCOL];
    if constexpr (NT > 0) {
        for (int i = threadIdx.x; i < NS * 64; i += 256) sU[i] = Up[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wv = threadIdx.x >> 6;
    const int nt = (K + 15) / 16;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    const int64_t nblk = (m + 15) / 16;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + wv; blk < nblk; blk += (int64_t)gridDim.x * 4) {
        const int64_t row = blk * 16 + e;
        const bool in = row < m;
        const int64_t rr = in ? row : 0;            // padding rows re-read row 0 (selected away)
        const double* src = A + rr * lda;
        d4 d = {0.0, 0.0, 0.0, 0.0};
        if constexpr (NT > 0) {
            d4u x[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) x[j] = sse_chunk(src, 16 * j + 4 * ks, K);
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    d = __builtin_amdgcn_mfma_f64_16x16x4f64(sU[(4 * j + t) * 64 + lane], x[j][t], d, 0, 0, 0);
        } else {
            for (int j = 0; j < nt; ++j) {
                const d4u x = sse_chunk(src, 16 * j + 4 * ks, K);
                const double* uj = Up + (int64_t)(4 * j) * 64 + lane;
#pragma unroll
                for (int t = 0; t < 4; ++t) d = __builtin_amdgcn_mfma_f64_16x16x4f64(uj[t * 64], x[t], d, 0, 0, 0);
            }
        }
        const bool keep = in && mask[rr] != 0;
        const double bb = b[rr], ww = w[rr];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double r = ww * (d[g] - bb);
            acc[g] = keep ? __builtin_fma(r, r, acc[g]) : acc[g];
        }
        cnt += keep ? 1.0 : 0.0;
    }
    // the 16 rows of a lane group (the same tree for every slot), then the four waves in a fixed order
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] += __shfl_xor(acc[g], o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (e == 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) fold[wv][ks + 4 * g] = acc[g];
    }
    if (lane == 0) fold[wv][fsnap::SSE_MAX_P] = cnt;
    __syncthreads();
    if (threadIdx.x < SSE_NCOL) {
        const int c = threadIdx.x;
        partial[(int64_t)blockIdx.x * SSE_NCOL + c] = (fold[0][c] + fold[1][c]) + (fold[2][c] + fold[3][c]);
    }
}

}  // namespace

namespace fsnap {

int sse_num_blocks(int64_t m) {
    int64_t nb = (m + 63) / 64;          // 64 rows per workgroup and step
    if (nb > 1024) nb = 1024;            // four waves per SIMD, a grid-stride loop over the rest
    if (nb < 1) nb = 1;
    return (int)nb;
}

void sse_pack_u(const double* U, int P, int K, double* Up) {
    const int ns = 4 * ((K + 15) / 16);
    for (int s = 0; s < ns; ++s)
        for (int ks = 0; ks < 4; ++ks)
            for (int p = 0; p < 16; ++p) {
                const int k = 16 * (s / 4) + 4 * ks + (s % 4);
                Up[(int64_t)s * 64 + ks * 16 + p] = (p < P && k < K) ? U[(int64_t)p * K + k] : 0.0;
            }
}

hipError_t launch_sse_batch(const double* A, int64_t lda, int64_t m, int K, const double* Up, const double* b, const double* w,
                            const unsigned char* mask, double* partial, double* out, hipStream_t st) {
    const int nb = sse_num_blocks(m);
    dispatch_nt((K + 15) / 16, [&](auto nt) {
        hipLaunchKernelGGL((fsnap_sse_rows_k<decltype(nt)::value>), dim3((unsigned)nb), dim3(256), 0, st, A, lda, m, K, Up, b, w, mask,
                           partial);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_colsum(partial, nb, SSE_NCOL, out, st);
}

}  // namespace fsnap
