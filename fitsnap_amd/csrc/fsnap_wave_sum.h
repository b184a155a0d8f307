// fsnap_wave_sum.h — wave reductions (and the lane broadcast) of the post-fit kernels, each in a fixed order: the order is part
// of every kernel's bit-identity promise.  (Kept out of fsnap_device_common.h: the recorded PMC traffic of the SYRK kernels,
// profiles/pmc_traffic.json, is keyed on that file's digest.)  Internal.
#pragma once
#include "fsnap_device_common.h"

// sum over the four lanes e, e + 16, e + 32, e + 48 of an MFMA k-slot group: xor 16, then xor 32
__device__ __forceinline__ double ks_sum(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
// sum over the 64 lanes of a wave, butterfly xor 1, 2, ..., 32
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the same sum with the butterfly run from xor 32 down to xor 1 (the order fsnap_cand.hip's chunk scalars are defined in)
__device__ __forceinline__ double wave_sum_desc(double v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// maximum over the 64 lanes of a wave
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// the value of lane `src` (uniform) in every lane
__device__ __forceinline__ double lane_bcast(double v, int src) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u & 0xFFFFFFFFull), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
