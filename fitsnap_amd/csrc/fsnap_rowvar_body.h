// fsnap_rowvar_body.h — device bodies shared by the predictive-variance kernels (fsnap_uq.hip: U1G, U2, U3) and the
// selection kernels that promise the same bits (fsnap_select.hip: B1G, B2, B3).  One body each, so the two sets cannot
// drift apart.  Internal.
#pragma once
#include "fsnap_device_common.h"
#include "fsnap_kernels.h"
#include "fsnap_wave_sum.h"

namespace fsnap_rowvar {

constexpr int RB = 2;   // 16-row blocks per wave

template <int MODE>
__device__ __forceinline__ double fold(double v, double t, double a) {
    if constexpr (MODE == fsnap::UQ_QUAD) return __builtin_fma(t, a, v);
    else return __builtin_fma(t, t, v);
}

// Any K (untuned): a wave takes RB blocks of 16 rows; the row values are loaded per k step of every M tile.
// SUB = false: var[i] = value (U1G); SUB = true: var[i] = var[i] - value (B1G).  256 threads per workgroup.
template <int MODE, bool SUB>
__device__ __forceinline__ void rows_gen_body(const double* __restrict__ A, int64_t lda, int64_t m, int K,
                                              const double* __restrict__ Mp, int Jp, const double* __restrict__ bp,
                                              double* __restrict__ var, double* __restrict__ preds) {
    const int lane = threadIdx.x & 63, e = lane & 15, ks = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RB);
    const int ns = (K + 3) / 4;
    const double* src[RB];
    int64_t row[RB];
    bool valid[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        row[r] = row0 + 16 * r + e;
        valid[r] = row[r] < m;
        src[r] = A + (valid[r] ? row[r] : 0) * lda;
    }
    auto ld = [&](int r, int k) -> double { return (valid[r] && k < K) ? src[r][k] : 0.0; };
    if (preds) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            double p = 0.0;
            for (int s = 0; s < ns; ++s) p = __builtin_fma(ld(r, 4 * s + ks), bp[4 * s + ks], p);
            p = ks_sum(p);
            if (ks == 0 && valid[r]) preds[row[r]] = p;
        }
    }
    if (!var) return;
    double v[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) v[r] = 0.0;
    const int njt = Jp / 16;
    for (int jt = 0; jt < njt; ++jt) {
        d4 acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = d4{0.0, 0.0, 0.0, 0.0};
        const double* mcol = Mp + 16 * jt + e;
        for (int s = 0; s < ns; ++s) {
            const double mf = mcol[(int64_t)(4 * s + ks) * Jp];
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(mf, ld(r, 4 * s + ks), acc[r], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                v[r] = fold<MODE>(v[r], acc[r][g], MODE == fsnap::UQ_QUAD ? ld(r, 16 * jt + ks + 4 * g) : 0.0);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const double s = ks_sum(v[r]);
        if (ks == 0 && valid[r]) {
            if constexpr (SUB) var[row[r]] = var[row[r]] - s;
            else var[row[r]] = s;
        }
    }
}

// One wave per chunk; lane l takes positions l, l + 64, ... of the chunk in order, then a fixed butterfly.
// part[chunk][2] = (sum, max) of s_i v_i over the chunk's rows (s = 1 without a scale).  alive (may be nullptr): a chunk of
// a category with alive[cat] == 0 keeps what it had.
__device__ __forceinline__ void chunk_body(const double* __restrict__ var, const double* __restrict__ scale,
                                           const int* __restrict__ idx, const fsnap::CatChunk* __restrict__ chunks,
                                           const int* __restrict__ alive, double* __restrict__ part) {
    const fsnap::CatChunk ch = chunks[blockIdx.x];
    if (alive && !alive[ch.cat]) return;
    const int lane = threadIdx.x;
    double s = 0.0, mx = -__builtin_inf();
    for (int p = lane; p < ch.count; p += 64) {
        const int r = idx[ch.first + p];
        const double val = scale ? scale[r] * var[r] : var[r];
        s += val;
        mx = val > mx ? val : mx;
    }
    for (int o = 1; o < 64; o <<= 1) {
        s += __shfl_xor(s, o, 64);
        const double om = __shfl_xor(mx, o, 64);
        mx = om > mx ? om : mx;
    }
    if (lane == 0) {
        part[2 * (int64_t)blockIdx.x] = s;
        part[2 * (int64_t)blockIdx.x + 1] = mx;
    }
}

// One thread per category (256 per workgroup), its chunks in order (cbeg[ncat + 1]); an empty category gets (0, -inf); with
// alive (may be nullptr) a category with alive[c] == 0 keeps what it had.  cat_sum / cat_max may be nullptr.
__device__ __forceinline__ void cat_body(const double* __restrict__ part, const int* __restrict__ cbeg,
                                         const int* __restrict__ alive, int ncat, double* __restrict__ cat_sum,
                                         double* __restrict__ cat_max) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncat || (alive && !alive[c])) return;
    double s = 0.0, mx = -__builtin_inf();
    for (int ch = cbeg[c]; ch < cbeg[c + 1]; ++ch) {
        s += part[2 * (int64_t)ch];
        const double om = part[2 * (int64_t)ch + 1];
        mx = om > mx ? om : mx;
    }
    if (cat_sum) cat_sum[c] = s;
    if (cat_max) cat_max[c] = mx;
}

}  // namespace fsnap_rowvar
