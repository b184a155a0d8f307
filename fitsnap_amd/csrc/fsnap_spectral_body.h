// fsnap_spectral_body.h — the statements of the spectral paths (include/fsnap_hip.h, fsnap_spectral_gram / fsnap_spectral_path)
// that the host route (fsnap_solve.cpp) and kernels E1 / E2 of fsnap_spectral.hip share, so that both evaluate one text: the
// round-robin pair ordering, the Jacobi rotation with its skip rule, the 2 x 2 block update, the order of the stopping sums and
// the per-setting filter.  Every product that feeds a sum is an explicit fma, so no compiler contracts the two routes
// differently.  Internal.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define FSNAP_SPEC_HD __host__ __device__ __forceinline__
#else
#define FSNAP_SPEC_HD inline
#endif

namespace fsnap {

constexpr int SPEC_MAX_SWEEPS = 60;            // jacobi_eigh's cap; reaching it is status 2
constexpr int SPEC_LANES = 1024;               // the stopping sums are taken as by the 1024 lanes (16 waves of 64) of kernel E1
constexpr double SPEC_SKIP = 1e-18;            // |a_pq| <= SPEC_SKIP sqrt(|a_pp| |a_qq|): set to zero, no rotation
constexpr double SPEC_STOP = 1e-34;            // off^2 <= SPEC_STOP diag^2: converged
constexpr double SPEC_EPS = 2.220446049250313e-16;

// Pair k (0 <= k < m / 2) of round r (0 <= r < m - 1) of the circle tournament on m players (m even): player m - 1 stays,
// the others turn.  p < q.  With an odd number n of rows m = n + 1 and the pair holding player n is a bye.
FSNAP_SPEC_HD void spec_pair(int m, int r, int k, int& p, int& q) {
    int a = m - 1, b = r;
    if (k > 0) {
        a = (r + k) % (m - 1);
        b = (r - k + (m - 1)) % (m - 1);
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

struct SpecRot {
    double c, s, t;        // identity: c = 1, s = t = 0
};

// The rotation that annihilates a_pq (jacobi_eigh's formula and skip rule).  The caller sets a_pq to zero in every case,
// a_pp -= t a_pq and a_qq += t a_pq.
FSNAP_SPEC_HD SpecRot spec_rot(double app, double aqq, double apq) {
    SpecRot r;
    r.c = 1.0;
    r.s = 0.0;
    r.t = 0.0;
    if (apq == 0.0 || fabs(apq) <= SPEC_SKIP * sqrt(fabs(app) * fabs(aqq))) return r;
    const double theta = (aqq - app) / (2.0 * apq);
    r.t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
    r.c = 1.0 / sqrt(fma(r.t, r.t, 1.0));
    r.s = r.t * r.c;
    return r;
}

// x' = c x - s y, y' = s x + c y: two rows of the eigenvector array, or one side of a block
FSNAP_SPEC_HD void spec_apply(double c, double s, double& x, double& y) {
    const double nx = fma(c, x, -(s * y)), ny = fma(s, x, c * y);
    x = nx;
    y = ny;
}

// B <- J_a^T B J_b for the 2 x 2 block of rows (p_a, q_a) and columns (p_b, q_b)
FSNAP_SPEC_HD void spec_block(double ca, double sa, double cb, double sb, double& b00, double& b01, double& b10, double& b11) {
    spec_apply(ca, sa, b00, b10);
    spec_apply(ca, sa, b01, b11);
    spec_apply(cb, sb, b00, b01);
    spec_apply(cb, sb, b10, b11);
}

// entry (i, j) of the packed lower triangle
FSNAP_SPEC_HD int spec_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// the lower pair index a of block e of the strictly lower triangle of pairs (e = a (a - 1) / 2 + b, b < a)
FSNAP_SPEC_HD int spec_block_row(int e) {
    int a = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)e)) * 0.5f);
    while (a * (a - 1) / 2 > e) --a;
    while ((a + 1) * a / 2 <= e) ++a;
    return a;
}

// cut of setting (alpha, rcond) on a problem with n_live columns: direction i is kept iff lambda_i > cut
FSNAP_SPEC_HD double spec_cut(double rcond, int n_live, double lmax) {
    const double r2 = rcond * rcond, fl = 4.0 * (double)n_live * SPEC_EPS;
    return (r2 > fl ? r2 : fl) * lmax;
}

// the filter factor of direction i: z_i / (lambda_i + alpha) when kept, 0 otherwise
FSNAP_SPEC_HD double spec_g(double lam, double z, double alpha, double cut) { return lam > cut ? z / (lam + alpha) : 0.0; }

struct SpecSet {
    double rank, dof, sse;
};

// rank, dof and sse of one setting from (lambda, z) ascending: one pass, i ascending
FSNAP_SPEC_HD SpecSet spec_setting(const double* lam, const double* z, int n, double alpha, double cut, double y2) {
    SpecSet r;
    r.rank = 0.0;
    r.dof = 0.0;
    double gz = 0.0, lgg = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!(lam[i] > cut)) continue;
        const double g = z[i] / (lam[i] + alpha);
        r.rank += 1.0;
        r.dof += lam[i] / (lam[i] + alpha);
        gz = fma(g, z[i], gz);
        lgg = fma(lam[i] * g, g, lgg);
    }
    const double sse = fma(-2.0, gz, y2) + lgg;
    r.sse = sse > 0.0 ? sse : 0.0;
    return r;
}

}  // namespace fsnap
