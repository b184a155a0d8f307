// fsnap_fold_body.h — the statements that the kernels of the grouped K-fold paths share ("The fold frame"): kernel
// S2 of fsnap_lasso.hip, A1 of fsnap_ard.hip and O1 of fsnap_omp.hip refit on "total minus fold f" of the packed blocks
// [G | c | bb, sum wb, n] that kernel S1 leaves (K^2 + K + 3 doubles each).  Here: the per-problem view of the two blocks, the
// dead-column rule and the held-out record -- what solvers/folds.py states on the host (downdated, and the heldout rows).  The
// solvers, their LDS layouts and their reduction orders are each kernel's own.  A shared piece must leave a kernel's registers,
// spills, LDS and occupancy as they were (scripts/kernel_resources.py): kernel O1 therefore keeps the view's statements as its
// own text.  Internal.
#pragma once
#include "fsnap_device_common.h"

// Problem f of F + 1: fold f left out (Gf: its block), or none (f = F: Gf = nullptr, the total alone).
struct FoldView {
    const double* Gf;
    double bb_f, n_f;      // the fold's own |y|^2 and row count (0 without a fold)
    double y2, n;          // of the rows that remain: total.bb - bb_f, total.n - n_f
};

__device__ __forceinline__ FoldView fold_view(const double* folds, const double* total, int f, int F, int K) {
    const int64_t T = (int64_t)K * K + K + 3;
    const int KK = K * K;
    FoldView v;
    v.Gf = f < F ? folds + (int64_t)f * T : nullptr;
    v.bb_f = v.Gf ? v.Gf[KK + K] : 0.0;
    v.n_f = v.Gf ? v.Gf[KK + K + 2] : 0.0;
    v.y2 = v.Gf ? total[KK + K] - v.bb_f : total[KK + K];
    v.n = v.Gf ? total[KK + K + 2] - v.n_f : total[KK + K + 2];
    return v;
}

// Column j takes no part in a refit -- skipped, coefficient 0 -- when the total never touched it (tjj = total G_jj = 0) or the
// subtraction left noise (qjj = downdated G_jj <= pivot_tol tjj).
__device__ __forceinline__ bool fold_dead(double tjj, double qjj, double pivot_tol) { return tjj == 0.0 || qjj <= pivot_tol * tjj; }

// The held-out record of fold f under its own refit: (n_f, h = bb_f - 2 beta . c_f + beta^T G_f beta, bb_f).
__device__ __forceinline__ void fold_heldout_store(double* ho, double n_f, double h, double bb_f) {
    ho[0] = n_f;
    ho[1] = h;
    ho[2] = bb_f;
}
