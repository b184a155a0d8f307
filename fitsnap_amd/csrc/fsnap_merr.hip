// fsnap_merr.hip — model-error (MERR) log-posterior and its exact gradient in one pass over the resident rows (gfx950 only):
//   M1  fsnap_merr_rows_k      K <= 288: one pass, a row is read once                 (lreg.py:66-123 logpost_emb)
//   M2  fsnap_merr_coef_k      K >  288: per-row (alpha w, beta w^2) to a 16 B/row buffer + per-workgroup value partials
//   M3  fsnap_merr_gemvT_k     K >  288: g = A^T (alpha w), h = (A o A)^T (beta w^2) in one transposed pass
// Notation (x_i = w_i a_i the weighted row, q_j = sigma_j^2, zero outside the embedded columns, d the data variance):
//     e_i = x_i . c - w_i b_i = w_i (a_i . c - b_i)       v_i = sum_j x_ij^2 q_j + d = w_i^2 (a_i^2 . q) + d
// Per training row the method gives the value term l_i and the two scalars alpha_i = dl/de, beta_i = dl/dv:
//     iid / full   l = -e^2 / (2 v) - log(v) / 2           alpha = -e / v        beta = e^2 / (2 v^2) - 1 / (2 v)
//     abc          r = |e| - sqrt(v), l = -r^2 / (2 eps^2) alpha = -r sign(e) / eps^2   beta = r / (2 eps^2 sqrt(v))
// and the pass returns  val = sum l_i,  g = sum alpha_i x_i = sum (alpha_i w_i) a_i,  h = sum beta_i x_i o x_i =
// sum (beta_i w_i^2) a_i o a_i.  The host adds the constants and composes the gradient in (c, s).  Training rows are those
// of the mask, whatever their weight: a row with w = 0 still contributes l(0, d).  Rows that do not take part (test rows,
// rows past m) are zeroed by selects: NaN / Inf in them reach nothing.  Partials: one row [g | h | val] (2K + 1 doubles)
// per workgroup, folded in a fixed order by fsnap_colsum_partials_k -- the result is bit-identical run to run.
#include "fsnap_device_common.h"
#include "fsnap_kernels.h"

namespace {

constexpr double kAbcEps = 0.1;     // lreg.py: abceps (abcalpha = 1)

// (l, alpha, beta) of one training row from e and v
__device__ __forceinline__ void merr_row_terms(int method, double e, double v, double& l, double& al, double& be) {
    if (method == fsnap::MERR_ABC) {
        const double sv = sqrt(v);
        const double r = __builtin_fabs(e) - sv;
        constexpr double ie2 = 1.0 / (kAbcEps * kAbcEps);
        l = -0.5 * r * r * ie2;
        const double sg = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
        al = -r * ie2 * sg;
        be = 0.5 * r * ie2 / sv;
    } else {                         // iid; full with the reference's diagonal covariance is the same density
        const double iv = 1.0 / v;
        const double ev = e * iv;
        l = -0.5 * e * ev - 0.5 * log(v);
        al = -ev;
        be = 0.5 * ev * ev - 0.5 * iv;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------
// Kernel M1: the one-pass form (K <= 32 NJ, NJ <= 9), the shape of kernel 4+7 (fsnap_residual_rows_k): 16 lanes per row,
// a lane owns the column pairs 2e + 32 j, a wave takes 8 rows per step (two groups of four).  Two dot products per row
// (a . c and a^2 . q), shuffle-reduced over the 16 lanes, then per-lane accumulators g += (alpha w) a, h += (beta w^2) a^2.
// HBM-bound: 8K + 17 bytes per row.
// ---------------------------------------------------------------------------------
template <int NJ>
struct MerrRows {
    d2u x[2][NJ];
    double bb[2], ww[2];
    bool keep[2];
};

template <int NJ>
__global__ __launch_bounds__(256) void fsnap_merr_rows_k(const double* __restrict__ A, int64_t lda,
                                                         const double* __restrict__ cq, int64_t m, int K,
                                                         const double* __restrict__ b, const double* __restrict__ w,
                                                         const unsigned char* __restrict__ mask, int method, double d,
                                                         double* __restrict__ partial) {
    constexpr int KP = NJ * 32;
    __shared__ __attribute__((aligned(16))) double scq[2][KP];
    __shared__ double fold[4][2 * KP];
    __shared__ double wsum[4];
    for (int i = threadIdx.x; i < KP; i += 256) {
        scq[0][i] = i < K ? cq[i] : 0.0;
        scq[1][i] = i < K ? cq[K + i] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, e = lane & 15, kr = lane >> 4, wv = threadIdx.x >> 6;
    bool v1[NJ], v2[NJ];
    int coff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = 2 * e + 32 * j;
        v1[j] = c < K;
        v2[j] = c + 1 < K;
        coff[j] = v1[j] ? c : 0;          // lanes past the row's end re-read its first pair (selected away)
    }
    double g0[NJ], g1[NJ], h0[NJ], h1[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) g0[j] = g1[j] = h0[j] = h1[j] = 0.0;
    double val = 0.0;
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv, step = (int64_t)gridDim.x * 4 * 8;

    auto fetch = [&](int64_t r0, MerrRows<NJ>& R) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t row = r0 + 4 * h + kr;
            const bool in = row < m;
            const int64_t rr = in ? row : 0;
            R.keep[h] = in && (mask[rr] != 0);
            R.bb[h] = b[rr];
            R.ww[h] = w[rr];
            const double* src = A + rr * lda;
#pragma unroll
            for (int j = 0; j < NJ; ++j) R.x[h][j] = __builtin_nontemporal_load(reinterpret_cast<const d2u*>(src + coff[j]));
        }
    };
    auto process = [&](const MerrRows<NJ>& R) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double x0[NJ], x1[NJ];
            double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const d2u cc = *reinterpret_cast<const d2u*>(&scq[0][2 * e + 32 * j]);
                const d2u qq = *reinterpret_cast<const d2u*>(&scq[1][2 * e + 32 * j]);
                x0[j] = (R.keep[h] && v1[j]) ? R.x[h][j][0] : 0.0;
                x1[j] = (R.keep[h] && v2[j]) ? R.x[h][j][1] : 0.0;
                s0 = __builtin_fma(x0[j], cc[0], s0);
                s1 = __builtin_fma(x1[j], cc[1], s1);
                t0 = __builtin_fma(x0[j] * x0[j], qq[0], t0);
                t1 = __builtin_fma(x1[j] * x1[j], qq[1], t1);
            }
            double sd = s0 + s1, td = t0 + t1;
            sd += __shfl_xor(sd, 8, 64);
            td += __shfl_xor(td, 8, 64);
            sd += __shfl_xor(sd, 4, 64);
            td += __shfl_xor(td, 4, 64);
            sd += __shfl_xor(sd, 2, 64);
            td += __shfl_xor(td, 2, 64);
            sd += __shfl_xor(sd, 1, 64);
            td += __shfl_xor(td, 1, 64);
            const double wr = R.keep[h] ? R.ww[h] : 0.0;
            const double er = R.keep[h] ? wr * (sd - R.bb[h]) : 0.0;
            const double vr = __builtin_fma(wr * wr, td, d);
            double l, al, be;
            merr_row_terms(method, er, vr, l, al, be);
            const double u = R.keep[h] ? al * wr : 0.0;
            const double u2 = R.keep[h] ? be * (wr * wr) : 0.0;
            if (e == 0 && R.keep[h]) val += l;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                g0[j] = __builtin_fma(x0[j], u, g0[j]);
                g1[j] = __builtin_fma(x1[j], u, g1[j]);
                h0[j] = __builtin_fma(x0[j] * x0[j], u2, h0[j]);
                h1[j] = __builtin_fma(x1[j] * x1[j], u2, h1[j]);
            }
        }
    };

    {                   // one register set: the waves of a SIMD cover each other's load latency
        MerrRows<NJ> R0;
        for (int64_t r0 = wave * 8; r0 < m; r0 += step) {
            fetch(r0, R0);
            process(R0);
        }
    }
    // fold: the four row groups of a wave (lanes e, e + 16, e + 32, e + 48), then the four waves through LDS, fixed order
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        g0[j] += __shfl_xor(g0[j], 16, 64);
        g0[j] += __shfl_xor(g0[j], 32, 64);
        g1[j] += __shfl_xor(g1[j], 16, 64);
        g1[j] += __shfl_xor(g1[j], 32, 64);
        h0[j] += __shfl_xor(h0[j], 16, 64);
        h0[j] += __shfl_xor(h0[j], 32, 64);
        h1[j] += __shfl_xor(h1[j], 16, 64);
        h1[j] += __shfl_xor(h1[j], 32, 64);
        if (kr == 0) {
            fold[wv][2 * e + 32 * j] = g0[j];
            fold[wv][2 * e + 32 * j + 1] = g1[j];
            fold[wv][KP + 2 * e + 32 * j] = h0[j];
            fold[wv][KP + 2 * e + 32 * j + 1] = h1[j];
        }
    }
    val += __shfl_xor(val, 16, 64);
    val += __shfl_xor(val, 32, 64);
    if (lane == 0) wsum[wv] = val;
    __syncthreads();
    double* out = partial + (int64_t)blockIdx.x * (2 * K + 1);
    for (int c = threadIdx.x; c < K; c += 256) {
        out[c] = (fold[0][c] + fold[1][c]) + (fold[2][c] + fold[3][c]);
        out[K + c] = (fold[0][KP + c] + fold[1][KP + c]) + (fold[2][KP + c] + fold[3][KP + c]);
    }
    if (threadIdx.x == 0) out[2 * K] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---------------------------------------------------------------------------------
// Kernel M2 (K > 288): one wave per row, the lanes stride over the columns; per training row u[i] = (alpha_i w_i,
// beta_i w_i^2), zeros elsewhere; value partials val_part[wg] (four waves folded in a fixed order).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fsnap_merr_coef_k(const double* __restrict__ A, int64_t lda,
                                                         const double* __restrict__ cq, int64_t m, int K,
                                                         const double* __restrict__ b, const double* __restrict__ w,
                                                         const unsigned char* __restrict__ mask, int method, double d,
                                                         double* __restrict__ u, double* __restrict__ val_part) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double val = 0.0;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < m; row += (int64_t)gridDim.x * 4) {
        const bool keep = mask[row] != 0;
        double s = 0.0, t = 0.0;
        if (keep) {
            const double* src = A + row * lda;
            for (int c = lane; c < K; c += 64) {
                const double x = src[c];
                s = __builtin_fma(x, cq[c], s);
                t = __builtin_fma(x * x, cq[K + c], t);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            t += __shfl_xor(t, o, 64);
        }
        const double wr = keep ? w[row] : 0.0;
        const double er = keep ? wr * (s - b[row]) : 0.0;
        const double vr = __builtin_fma(wr * wr, t, d);
        double l, al, be;
        merr_row_terms(method, er, vr, l, al, be);
        if (lane == 0) {
            u[2 * row] = keep ? al * wr : 0.0;
            u[2 * row + 1] = keep ? be * (wr * wr) : 0.0;
            if (keep) val += l;
        }
    }
    if (lane == 0) wsum[wv] = val;
    __syncthreads();
    if (threadIdx.x == 0) val_part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---------------------------------------------------------------------------------
// Kernel M3 (K > 288): the two transposed products in one pass.  A workgroup owns a row range and writes one partial row
// [g | h | val] (val from kernel M2's val_part[wg]); a thread owns the columns tid, tid + 256, ... and walks the rows of
// the range (the 256 threads of a row read it coalesced).  Test rows are selected away: NaN / Inf in them reach nothing.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fsnap_merr_gemvT_k(const double* __restrict__ A, int64_t lda,
                                                          const double* __restrict__ u, const unsigned char* __restrict__ mask,
                                                          int64_t m, int K, int64_t rows_per_wg,
                                                          const double* __restrict__ val_part, double* __restrict__ partial) {
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
    int64_t r1 = r0 + rows_per_wg;
    if (r1 > m) r1 = m;
    double* out = partial + (int64_t)blockIdx.x * (2 * K + 1);
    for (int c = threadIdx.x; c < K; c += 256) {
        double ga = 0.0, ha = 0.0;
        for (int64_t row = r0; row < r1; ++row) {
            const bool keep = mask[row] != 0;
            const double x = keep ? A[row * lda + c] : 0.0;
            ga = __builtin_fma(x, u[2 * row], ga);
            ha = __builtin_fma(x * x, u[2 * row + 1], ha);
        }
        out[c] = ga;
        out[K + c] = ha;
    }
    if (threadIdx.x == 0) out[2 * K] = val_part[blockIdx.x];
}

namespace fsnap {

// workgroups of kernel M1: one resident round of the chip, as kernel 4+7 (residual_num_blocks), by the waves per SIMD
// of the instantiation (4 / 3 / 2 / 2 / 2 / 1 / 1 / 1 for NJ = 1 / 2 / 3 / 4 / 5 / 6 / 8 / 9; no scratch)
int merr_num_blocks(int64_t m, int K) {
    if (K > MERR_ONE_PASS_MAX_K) {
        int64_t nb = (m + 255) / 256;
        if (nb > 2048) nb = 2048;
        if (nb < 1) nb = 1;
        return (int)nb;
    }
    const int nj = (K + 31) / 32;
    const int per_cu = nj <= 1 ? 4 : nj == 2 ? 3 : nj <= 5 ? 2 : 1;
    int64_t nb = (m + 31) / 32;
    if (nb > 256 * per_cu) nb = 256 * per_cu;
    if (nb < 1) nb = 1;
    return (int)nb;
}

hipError_t launch_merr(const double* A, int64_t lda, const double* cq, int64_t m, int K, const double* b, const double* w,
                       const unsigned char* mask, int method, double d, double* u, double* val_part, double* partial,
                       double* out, hipStream_t st) {
    const int nb = merr_num_blocks(m, K);
    if (K > MERR_ONE_PASS_MAX_K) {
        const int64_t rpw = (m + nb - 1) / nb;
        hipLaunchKernelGGL(fsnap_merr_coef_k, dim3((unsigned)nb), dim3(256), 0, st, A, lda, cq, m, K, b, w, mask, method, d,
                           u, val_part);
        hipLaunchKernelGGL(fsnap_merr_gemvT_k, dim3((unsigned)nb), dim3(256), 0, st, A, lda, u, mask, m, K, rpw, val_part,
                           partial);
    } else {
        const int nj = (K + 31) / 32;
#define FSNAP_LAUNCH(NJ) \
        hipLaunchKernelGGL((fsnap_merr_rows_k<NJ>), dim3((unsigned)nb), dim3(256), 0, st, A, lda, cq, m, K, b, w, mask, method, d, partial)
        switch (nj) {
            case 1: FSNAP_LAUNCH(1); break;
            case 2: FSNAP_LAUNCH(2); break;
            case 3: FSNAP_LAUNCH(3); break;
            case 4: FSNAP_LAUNCH(4); break;
            case 5: FSNAP_LAUNCH(5); break;
            case 6: FSNAP_LAUNCH(6); break;
            case 7: case 8: FSNAP_LAUNCH(8); break;
            case 9: FSNAP_LAUNCH(9); break;
            default: return hipErrorInvalidValue;
        }
#undef FSNAP_LAUNCH
    }
    return launch_colsum(partial, nb, 2 * K + 1, out, st);
}

}  // namespace fsnap
