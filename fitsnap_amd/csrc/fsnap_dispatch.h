// fsnap_dispatch.h — host helpers that turn a runtime kernel class into a compile-time constant for a generic lambda:
//     dispatch_nt(NT, [&](auto nt) { constexpr int N = decltype(nt)::value; kernel<N><<<...>>>(...); });
// Internal.
#pragma once
#include <type_traits>

namespace fsnap {

// f(integral_constant<int, nt>) for nt = ceil(K / 16) in 1 ... 9 (the register-resident kernels), f(<0>) for any other
template <class F>
inline void dispatch_nt(int nt, F&& f) {
    switch (nt) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 9: f(std::integral_constant<int, 9>{}); break;
        default: f(std::integral_constant<int, 0>{});
    }
}

// f(integral_constant<int, D>) for the solve-size bins D = 32, 64, 128 (LDS) and 0 (global scratch); false for any other D
template <class F>
inline bool dispatch_d(int D, F&& f) {
    switch (D) {
        case 32: f(std::integral_constant<int, 32>{}); return true;
        case 64: f(std::integral_constant<int, 64>{}); return true;
        case 128: f(std::integral_constant<int, 128>{}); return true;
        case 0: f(std::integral_constant<int, 0>{}); return true;
        default: return false;
    }
}

}  // namespace fsnap
