// fsnap_cand.hip — batched candidate fits of a weight search from per-category statistics (gfx950 only).
//
// A candidate p scales the base weight w0_i of every row of category c by S[p, c].  Its normal equations are then
//     G_p = sum_c S[p,c]^2 G_c,   c_p = sum_c S[p,c]^2 r_c,   G_c = sum_{i in c, training} w0_i^2 a_i a_i^T, r_c likewise
// so one pass over the rows gives every candidate's statistics, and one more pass gives the residual sums of P
// coefficient vectors at once.
//
// Work layout shared by the row kernels: the host stable-sorts the row ids by category (counting sort) and cuts every
// category into chunks of at most CAT_CHUNK_ROWS rows (CatChunk: category, first index, count).  A workgroup takes one
// chunk and gathers its rows through the sorted index; a stable sort keeps the rows of one configuration adjacent, so
// the gather reads mostly sequential runs.  Every workgroup (or wave) writes its own partial; the reductions below sum
// the partials of a category in chunk order.  No floating-point atomics: results are run-to-run bit-identical, and a
// candidate's result does not depend on the other candidates of its batch.
//
//   C1  fsnap_cat_syrk_k<NT>     K <= 144: per-chunk [G tiles | c | b^T W^2 b, sum wb, n] on v_mfma_f64_16x16x4_f64; the
//                                four waves of a workgroup share the chunk's rows and split the tile triangle; the register
//                                w0 a[row][16 t + e] is the A operand of tile (t, .) and the B operand of tile (., t)
//   C1G fsnap_cat_syrk_gen_k     K > 144 (untuned): one tile pair per wave, grid (pair groups, chunks)
//   C1R fsnap_cat_reduce_k       per-category packed [G | c | scalars] from the chunk partials (fixed order)
//   C2  fsnap_cand_combine_k     G_p, c_p, scalars_p = sum_c coef(S[p,c]) stats_c for P candidates (VALU, c in fixed order)
//   C3  fsnap_cand_rows_k<WHAT>  y = a . beta_p on the matrix pipe, 16 rows x 16 candidates per tile, then
//                                WHAT = 0: per (candidate, chunk) sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2, r = t - y
//                                WHAT = 1: s = A^T (w0^2 r) per chunk, the A fragments of the transposed product are the
//                                          rows of the 16-row block, the residual tile is the B operand as it stands
//   C3R fsnap_cand_reduce_k      WHAT = 0: per (candidate, category) sums; WHAT = 1: s_p = sum_c S[p,c]^2 s_c
#include <utility>

#include "fsnap_device_common.h"
#include "fsnap_dispatch.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace {

using fsnap::CatChunk;

__host__ __device__ constexpr int cat_tri(int p, int q, int NT) { return p * NT - (p * (p - 1)) / 2 + (q - p); }
__host__ __device__ constexpr int cat_pair_p(int k, int NT) {
    int p = 0;
    while (k >= NT - p) {
        k -= NT - p;
        ++p;
    }
    return p;
}
__host__ __device__ constexpr int cat_pair_q(int k, int NT) {
    int p = 0;
    while (k >= NT - p) {
        k -= NT - p;
        ++p;
    }
    return p + k;
}

template <class F, int... I>
__device__ __forceinline__ void cat_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void cat_for(F&& f) {
    cat_for_impl(f, std::make_integer_sequence<int, N>{});
}

// offset of G[i][j] (i <= j) inside one chunk's tile partials [pair][reg][lane]: D row = (lane >> 4) + 4 reg, col = lane & 15
__device__ __forceinline__ int64_t cat_tile_offset(int i, int j, int NT) {
    const int k = cat_tri(i >> 4, j >> 4, NT), r = i & 15;
    return (int64_t)k * 256 + (r >> 2) * 64 + (r & 3) * 16 + (j & 15);
}

// ---------------------------------------------------------------------------------
// Kernel C1: wave W owns the tile pairs k = W, W + 4, ... of the NT x NT triangle; all four waves stream the chunk's rows
// 4 at a time (lane: row slot lane >> 4, column e = lane & 15 of every 16-column tile).  The wave that owns the diagonal
// tile (t, t) also accumulates c over tile t; the owner of pair 0 the three scalars.
// ---------------------------------------------------------------------------------
template <int NT, int W>
__device__ __forceinline__ void cat_syrk_wave(const double* __restrict__ A, int64_t lda, const double* __restrict__ b,
                                              const double* __restrict__ w0, const int* __restrict__ idx, const CatChunk ch,
                                              int K, int64_t chunk, double* __restrict__ part, double* __restrict__ cpart,
                                              double* __restrict__ spart) {
    constexpr int NP = NT * (NT + 1) / 2;
    constexpr int NPW = (NP - W + 3) / 4;
    constexpr int NA = NPW > 0 ? NPW : 1;
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4;
    d4 acc[NA];
    double cacc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        acc[j] = d4{0.0, 0.0, 0.0, 0.0};
        cacc[j] = 0.0;
    }
    double s_bb = 0.0, s_b = 0.0, s_n = 0.0;
    for (int s = 0; s < ch.count; s += 4) {
        const int pos = s + ks;
        const bool valid = pos < ch.count;
        const int64_t r = idx[ch.first + (valid ? pos : 0)];
        const double wv = valid ? w0[r] : 0.0;
        const double* src = A + r * lda;
        double x[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = 16 * t + e;
            double v = 0.0;
            if (col < K) v = src[col];
            x[t] = valid ? wv * v : 0.0;
        }
        const double wb = valid ? wv * b[r] : 0.0;
        cat_for<NPW>([&](auto J) {
            constexpr int k = W + 4 * decltype(J)::value;
            constexpr int p = cat_pair_p(k, NT), q = cat_pair_q(k, NT);
            acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[p], x[q], acc[J], 0, 0, 0);
            if constexpr (p == q) cacc[J] = __builtin_fma(x[p], wb, cacc[J]);
        });
        if constexpr (W == 0) {
            if (e == 0) {
                s_bb = __builtin_fma(wb, wb, s_bb);
                s_b += wb;
                s_n += valid ? 1.0 : 0.0;
            }
        }
    }
    double* pc = part + chunk * (int64_t)NP * 256;
    cat_for<NPW>([&](auto J) {
        constexpr int k = W + 4 * decltype(J)::value;
        constexpr int p = cat_pair_p(k, NT), q = cat_pair_q(k, NT);
#pragma unroll
        for (int g = 0; g < 4; ++g) pc[k * 256 + g * 64 + lane] = acc[J][g];
        if constexpr (p == q) {
            const double v = ks_sum(cacc[J]);
            if (ks == 0) cpart[chunk * NT * 16 + 16 * p + e] = v;
        }
    });
    if constexpr (W == 0) {
        s_bb = wave_sum_desc(s_bb);
        s_b = wave_sum_desc(s_b);
        s_n = wave_sum_desc(s_n);
        if (lane == 0) {
            spart[chunk * 3 + 0] = s_bb;
            spart[chunk * 3 + 1] = s_b;
            spart[chunk * 3 + 2] = s_n;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) void fsnap_cat_syrk_k(const double* __restrict__ A, int64_t lda, const double* __restrict__ b,
                                                        const double* __restrict__ w0, const int* __restrict__ idx,
                                                        const CatChunk* __restrict__ chunks, int K, double* __restrict__ part,
                                                        double* __restrict__ cpart, double* __restrict__ spart) {
    const int64_t chunk = blockIdx.x;
    const CatChunk ch = chunks[chunk];
    switch (threadIdx.x >> 6) {
        case 0: cat_syrk_wave<NT, 0>(A, lda, b, w0, idx, ch, K, chunk, part, cpart, spart); break;
        case 1: cat_syrk_wave<NT, 1>(A, lda, b, w0, idx, ch, K, chunk, part, cpart, spart); break;
        case 2: cat_syrk_wave<NT, 2>(A, lda, b, w0, idx, ch, K, chunk, part, cpart, spart); break;
        default: cat_syrk_wave<NT, 3>(A, lda, b, w0, idx, ch, K, chunk, part, cpart, spart); break;
    }
}

// Kernel C1G (K > 144, untuned): wave k = 4 blockIdx.x + wave owns tile pair k; same partial layout as C1
__global__ __launch_bounds__(256) void fsnap_cat_syrk_gen_k(const double* __restrict__ A, int64_t lda,
                                                            const double* __restrict__ b, const double* __restrict__ w0,
                                                            const int* __restrict__ idx, const CatChunk* __restrict__ chunks,
                                                            int K, int NT, double* __restrict__ part,
                                                            double* __restrict__ cpart, double* __restrict__ spart) {
    const int NP = NT * (NT + 1) / 2;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= NP) return;
    const int64_t chunk = blockIdx.y;
    const CatChunk ch = chunks[chunk];
    const int p = cat_pair_p(k, NT), q = cat_pair_q(k, NT);
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4;
    const int cp = 16 * p + e, cq = 16 * q + e;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    double cacc = 0.0, s_bb = 0.0, s_b = 0.0, s_n = 0.0;
    for (int s = 0; s < ch.count; s += 4) {
        const int pos = s + ks;
        const bool valid = pos < ch.count;
        const int64_t r = idx[ch.first + (valid ? pos : 0)];
        const double wv = valid ? w0[r] : 0.0;
        const double* src = A + r * lda;
        double vp = 0.0, vq = 0.0;
        if (cp < K) vp = src[cp];
        if (cq < K) vq = src[cq];
        const double xp = valid ? wv * vp : 0.0, xq = valid ? wv * vq : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xp, xq, acc, 0, 0, 0);
        if (p == q) {
            const double wb = valid ? wv * b[r] : 0.0;
            cacc = __builtin_fma(xp, wb, cacc);
            if (k == 0 && e == 0) {
                s_bb = __builtin_fma(wb, wb, s_bb);
                s_b += wb;
                s_n += valid ? 1.0 : 0.0;
            }
        }
    }
    double* pc = part + chunk * (int64_t)NP * 256 + (int64_t)k * 256;
#pragma unroll
    for (int g = 0; g < 4; ++g) pc[g * 64 + lane] = acc[g];
    if (p == q) {
        cacc = ks_sum(cacc);
        if (ks == 0) cpart[chunk * NT * 16 + cp] = cacc;
    }
    if (k == 0) {
        s_bb = wave_sum_desc(s_bb);
        s_b = wave_sum_desc(s_b);
        s_n = wave_sum_desc(s_n);
        if (lane == 0) {
            spart[chunk * 3 + 0] = s_bb;
            spart[chunk * 3 + 1] = s_b;
            spart[chunk * 3 + 2] = s_n;
        }
    }
}

// Kernel C1R: stats[c][T] (T = K^2 + K + 3, the packed layout of fsnap_normal_eq_resident) = sum over the chunks of
// category c, in chunk order.  grid (ceil(T / 256), ncat)
__global__ __launch_bounds__(256) void fsnap_cat_reduce_k(const double* __restrict__ part, const double* __restrict__ cpart,
                                                          const double* __restrict__ spart, const int* __restrict__ cbeg,
                                                          int K, int NT, double* __restrict__ stats) {
    const int64_t T = (int64_t)K * K + K + 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T) return;
    const int c = blockIdx.y;
    const int NP = NT * (NT + 1) / 2;
    const int c0 = cbeg[c], c1 = cbeg[c + 1];
    double s = 0.0;
    if (e < (int64_t)K * K) {
        const int i = (int)(e / K), j = (int)(e % K);
        const int64_t off = cat_tile_offset(i < j ? i : j, i < j ? j : i, NT);
        for (int ch = c0; ch < c1; ++ch) s += part[(int64_t)ch * NP * 256 + off];
    } else if (e < (int64_t)K * K + K) {
        const int64_t j = e - (int64_t)K * K;
        for (int ch = c0; ch < c1; ++ch) s += cpart[(int64_t)ch * NT * 16 + j];
    } else {
        const int64_t j = e - (int64_t)K * K - K;
        for (int ch = c0; ch < c1; ++ch) s += spart[(int64_t)ch * 3 + j];
    }
    stats[(int64_t)c * T + e] = s;
}

// Kernel C2: out[p][e] = sum_c coef * stats[c][e], c = 0 .. ncat-1 in order; coef = S^2 (G, c, b^T W^2 b), S (sum wb),
// 1 (training-row count).  A thread keeps CAND_COMBINE_P candidates.  grid (ceil(T / 256), ceil(P / CAND_COMBINE_P))
constexpr int CAND_COMBINE_P = 8;
__global__ __launch_bounds__(256) void fsnap_cand_combine_k(const double* __restrict__ stats, const double* __restrict__ S,
                                                            int P, int ncat, int K, double* __restrict__ out) {
    const int64_t T = (int64_t)K * K + K + 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T) return;
    const int p0 = blockIdx.y * CAND_COMBINE_P;
    const int kind = e < T - 2 ? 2 : (e == T - 2 ? 1 : 0);
    double acc[CAND_COMBINE_P];
#pragma unroll
    for (int i = 0; i < CAND_COMBINE_P; ++i) acc[i] = 0.0;
    for (int c = 0; c < ncat; ++c) {
        const double v = stats[(int64_t)c * T + e];
#pragma unroll
        for (int i = 0; i < CAND_COMBINE_P; ++i) {
            const double s = p0 + i < P ? S[(int64_t)(p0 + i) * ncat + c] : 0.0;
            const double coef = kind == 2 ? s * s : (kind == 1 ? s : 1.0);
            acc[i] = __builtin_fma(coef, v, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < CAND_COMBINE_P; ++i)
        if (p0 + i < P) out[(int64_t)(p0 + i) * T + e] = acc[i];
}

// ---------------------------------------------------------------------------------
// Kernel C3: a workgroup takes one chunk, each wave 16-row blocks of it (block wave, wave + 4, ...).  Forward product
// y[16 rows][16 candidates] with 2 MFMAs per 8 columns: lane (row e, slot ks) holds a[row][k0 + 2 ks + {0, 1}] (16-byte
// runs of the row), betaT[k][16] (zero-padded to a multiple of 8 rows and to 16 candidates) gives the matching B slots.
// The result tile holds y[row ks + 4 g][candidate e] in register g.
//   WHAT = 0 (all rows of the chunk list): per lane four sums for candidate e; partial[chunk * 4 + wave][4][16]
//   WHAT = 1 (training rows): u = w0^2 (t - y) in the tile's own layout is the B operand B[slot ks][cand e] of
//            s[16 kt + i][e] += sum_slots a[row ks + 4 g][16 kt + i] u[row ks + 4 g][e], g = 0 .. 3; the wave keeps the
//            CAND_NTB tiles kt = CAND_NTB blockIdx.y + j; partial[chunk * 4 + wave][NT][4][64]
// ---------------------------------------------------------------------------------
constexpr int CAND_NTB = 9;

template <int WHAT>
__global__ __launch_bounds__(256) void fsnap_cand_rows_k(const double* __restrict__ A, int64_t lda, const double* __restrict__ b,
                                                         const double* __restrict__ w0, const int* __restrict__ idx,
                                                         const CatChunk* __restrict__ chunks, int K,
                                                         const double* __restrict__ betaT, double* __restrict__ partial) {
    const int64_t chunk = blockIdx.x;
    const CatChunk ch = chunks[chunk];
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int NT = (K + 15) / 16;
    const int kt0 = blockIdx.y * CAND_NTB;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    d4 acc[CAND_NTB];
#pragma unroll
    for (int j = 0; j < CAND_NTB; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    const int nblk = (ch.count + 15) / 16;
    for (int rb = wave; rb < nblk; rb += 4) {
        const int pos = rb * 16 + e;
        const bool valid = pos < ch.count;
        const int r32 = idx[ch.first + (valid ? pos : 0)];
        const double* src = A + (int64_t)r32 * lda;
        d4 y = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < K; k0 += 8) {
            const int kk = k0 + 2 * ks;
            double a0 = 0.0, a1 = 0.0;
            if (valid && kk < K) a0 = src[kk];
            if (valid && kk + 1 < K) a1 = src[kk + 1];
            const double b0 = betaT[(int64_t)kk * 16 + e], b1 = betaT[(int64_t)(kk + 1) * 16 + e];
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, y, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, y, 0, 0, 0);
        }
        const double t = valid ? b[r32] : 0.0, wv = valid ? w0[r32] : 0.0;
        const int vi = valid ? 1 : 0;
        double u[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int sl = ks + 4 * g;
            const double tr = __shfl(t, sl, 64), wr = __shfl(wv, sl, 64);
            const bool vr = __shfl(vi, sl, 64) != 0;
            const double res = tr - y[g];
            if constexpr (WHAT == 0) {
                if (vr) {
                    const double wres = wr * res;
                    s0 += __builtin_fabs(res);
                    s1 = __builtin_fma(res, res, s1);
                    s2 += __builtin_fabs(wres);
                    s3 = __builtin_fma(wres, wres, s3);
                }
            } else {
                u[g] = vr ? (wr * wr) * res : 0.0;
            }
        }
        if constexpr (WHAT == 1) {
            int rr[4];
            bool vv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                rr[g] = __shfl(r32, ks + 4 * g, 64);
                vv[g] = __shfl(vi, ks + 4 * g, 64) != 0;
            }
#pragma unroll
            for (int j = 0; j < CAND_NTB; ++j) {
                const int kt = kt0 + j;
                if (kt >= NT) break;
                const int col = 16 * kt + e;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    double av = 0.0;
                    if (vv[g] && col < K) av = A[(int64_t)rr[g] * lda + col];
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, u[g], acc[j], 0, 0, 0);
                }
            }
        }
    }
    const int64_t slot = chunk * 4 + wave;
    if constexpr (WHAT == 0) {
        double v[4] = {s0, s1, s2, s3};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = ks_sum(v[q]);
            if (ks == 0) partial[(slot * 4 + q) * 16 + e] = v[q];
        }
    } else {
#pragma unroll
        for (int j = 0; j < CAND_NTB; ++j) {
            const int kt = kt0 + j;
            if (kt >= NT) break;
#pragma unroll
            for (int g = 0; g < 4; ++g) partial[slot * NT * 256 + (int64_t)kt * 256 + g * 64 + lane] = acc[j][g];
        }
    }
}

// Kernel C3R, WHAT = 0: sums[(p0 + p) * ncat + c][4] = sum over the chunks of c and their four waves (fixed order).
// thread = (c, p, q); grid ceil(ncat * np * 4 / 256)
__global__ __launch_bounds__(256) void fsnap_cand_reduce_sums_k(const double* __restrict__ partial, const int* __restrict__ cbeg,
                                                                int ncat, int np, int p0, double* __restrict__ sums) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= (int64_t)ncat * np * 4) return;
    const int q = (int)(tid & 3), p = (int)((tid >> 2) % np), c = (int)(tid / (4 * np));
    double s = 0.0;
    for (int ch = cbeg[c]; ch < cbeg[c + 1]; ++ch)
        for (int wv = 0; wv < 4; ++wv) s += partial[(((int64_t)ch * 4 + wv) * 4 + q) * 16 + p];
    sums[((int64_t)(p0 + p) * ncat + c) * 4 + q] = s;
}

// Kernel C3R, WHAT = 1: rhs[(p0 + p)][k] = sum_c S[p0 + p][c]^2 (sum over the chunks of c and their waves).
// thread = (p, k); grid ceil(np * K / 256)
__global__ __launch_bounds__(256) void fsnap_cand_reduce_rhs_k(const double* __restrict__ partial, const int* __restrict__ cbeg,
                                                               const double* __restrict__ S, int ncat, int np, int p0, int K,
                                                               double* __restrict__ rhs) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= (int64_t)np * K) return;
    const int k = (int)(tid % K), p = (int)(tid / K);
    const int NT = (K + 15) / 16, r = k & 15;
    const int64_t off = (int64_t)(k >> 4) * 256 + (r >> 2) * 64 + (r & 3) * 16 + p;
    double s = 0.0;
    for (int c = 0; c < ncat; ++c) {
        double sc = 0.0;
        for (int ch = cbeg[c]; ch < cbeg[c + 1]; ++ch)
            for (int wv = 0; wv < 4; ++wv) sc += partial[((int64_t)ch * 4 + wv) * NT * 256 + off];
        const double sv = S[(int64_t)(p0 + p) * ncat + c];
        s = __builtin_fma(sv * sv, sc, s);
    }
    rhs[(int64_t)(p0 + p) * K + k] = s;
}

}  // namespace

namespace fsnap {

int cat_partial_doubles(int K) {
    const int NT = (K + 15) / 16;
    return NT * (NT + 1) / 2 * 256 + NT * 16 + 3;
}

hipError_t launch_cat_syrk(const double* A, int64_t lda, const double* b, const double* w0, const int* idx,
                           const CatChunk* chunks, int64_t nchunks, int K, double* part, double* cpart, double* spart,
                           hipStream_t st) {
    if (nchunks <= 0) return hipSuccess;
    const int NT = (K + 15) / 16;
    const dim3 grid((unsigned)nchunks);
    dispatch_nt(NT, [&](auto nt) {
        constexpr int N = decltype(nt)::value;
        if constexpr (N > 0) {
            fsnap_cat_syrk_k<N><<<grid, 256, 0, st>>>(A, lda, b, w0, idx, chunks, K, part, cpart, spart);
        } else {
            const int NP = NT * (NT + 1) / 2;
            fsnap_cat_syrk_gen_k<<<dim3((unsigned)((NP + 3) / 4), (unsigned)nchunks), 256, 0, st>>>(A, lda, b, w0, idx, chunks, K, NT,
                                                                                                  part, cpart, spart);
        }
    });
    return hipGetLastError();
}

hipError_t launch_cat_reduce(const double* part, const double* cpart, const double* spart, const int* cbeg, int ncat, int K,
                             double* stats, hipStream_t st) {
    const int64_t T = (int64_t)K * K + K + 3;
    fsnap_cat_reduce_k<<<dim3((unsigned)((T + 255) / 256), (unsigned)ncat), 256, 0, st>>>(part, cpart, spart, cbeg, K,
                                                                                         (K + 15) / 16, stats);
    return hipGetLastError();
}

hipError_t launch_cand_combine(const double* stats, const double* S, int P, int ncat, int K, double* out, hipStream_t st) {
    const int64_t T = (int64_t)K * K + K + 3;
    fsnap_cand_combine_k<<<dim3((unsigned)((T + 255) / 256), (unsigned)((P + CAND_COMBINE_P - 1) / CAND_COMBINE_P)), 256, 0, st>>>(
        stats, S, P, ncat, K, out);
    return hipGetLastError();
}

int64_t cand_rows_partial_doubles(int what, int K) { return what == 0 ? 4 * 4 * 16 : 4 * (int64_t)((K + 15) / 16) * 256; }

hipError_t launch_cand_rows(int what, const double* A, int64_t lda, const double* b, const double* w0, const int* idx,
                            const CatChunk* chunks, int64_t nchunks, int K, const double* betaT, double* partial,
                            hipStream_t st) {
    if (nchunks <= 0) return hipSuccess;
    if (what == 0) {
        fsnap_cand_rows_k<0><<<dim3((unsigned)nchunks), 256, 0, st>>>(A, lda, b, w0, idx, chunks, K, betaT, partial);
    } else {
        const int NT = (K + 15) / 16;
        fsnap_cand_rows_k<1><<<dim3((unsigned)nchunks, (unsigned)((NT + CAND_NTB - 1) / CAND_NTB)), 256, 0, st>>>(
            A, lda, b, w0, idx, chunks, K, betaT, partial);
    }
    return hipGetLastError();
}

hipError_t launch_cand_reduce(int what, const double* partial, const int* cbeg, const double* S, int ncat, int np, int p0,
                              int K, double* out, hipStream_t st) {
    if (what == 0) {
        const int64_t n = (int64_t)ncat * np * 4;
        fsnap_cand_reduce_sums_k<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(partial, cbeg, ncat, np, p0, out);
    } else {
        const int64_t n = (int64_t)np * K;
        fsnap_cand_reduce_rhs_k<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(partial, cbeg, S, ncat, np, p0, K, out);
    }
    return hipGetLastError();
}

}  // namespace fsnap
