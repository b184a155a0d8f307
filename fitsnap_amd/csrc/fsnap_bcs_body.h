// fsnap_bcs_body.h — the per-column statements of the BCS recurrence (fast relevance-vector machine of Tipping & Faul as coded
// by Ji; include/fsnap_hip.h, fsnap_bcs_gram) that the host route (fsnap_solve.cpp) and kernel B1 (fsnap_bcs.hip) share, so
// that both evaluate one text: the initial ratio, the noise rule and the three marginal-likelihood formulas.  The two routes
// still differ in the last bits of `log` and in the order of a few sums.  Internal.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define FSNAP_BCS_HD __host__ __device__ __forceinline__
#else
#define FSNAP_BCS_HD inline
#endif

namespace fsnap {

constexpr double BCS_NUGGET = 1e-16;
constexpr int BCS_RE = 0, BCS_ADD = 1, BCS_DEL = 2, BCS_STOP = 3;     // the action of a pick

// the score of the initial column
FSNAP_BCS_HD double bcs_ratio(double qj, double qjj) { return (qj * qj + BCS_NUGGET) / (qjj + BCS_NUGGET); }

// sigma2 = max(scale var(y), nugget) from the scalars of the rows (NaN, as with no rows, gives the nugget)
FSNAP_BCS_HD double bcs_sigma2(double scale, double y2, double sum_y, double n) {
    const double mean = sum_y / n;
    const double v = scale * (y2 / n - mean * mean);
    return v > BCS_NUGGET ? v : BCS_NUGGET;
}

struct BcsScore {
    double ml, theta, ss;      // ml = -inf: not a candidate; a NaN is one, and wins (numpy's argmax)
};

// Column j with S_j = s, Q_j = q; active with precision alpha, or inactive (can_add: the active set has room).
FSNAP_BCS_HD BcsScore bcs_score(double s, double q, bool active, double alpha, bool can_add) {
    BcsScore r;
    double qq = q;
    r.ss = s;
    if (active) {
        r.ss = alpha * s / (alpha - s);
        qq = alpha * q / (alpha - s);
    }
    r.theta = qq * qq - r.ss;
    r.ml = -HUGE_VAL;
    if (r.theta > 0.0) {
        if (active) {                                                 // re-estimate
            const double a_new = r.ss * r.ss / r.theta + BCS_NUGGET;
            const double delta = (alpha - a_new) / (a_new * alpha);
            r.ml = q * q * delta / (s * delta + 1.0) - log(1.0 + s * delta);
        } else if (can_add) {                                         // add
            r.ml = (q * q - s) / s + log(s / (q * q));
        }
    } else if (active) {                                              // delete
        r.ml = q * q / (s - alpha) - log(1.0 - s / alpha);
    }
    return r;
}

// numpy's argmax order: (ov, oi) goes before (v, i) when ov is larger, a NaN being larger than every number, or on equality
// (two NaNs are equal) when its index is lower
FSNAP_BCS_HD bool bcs_before(double ov, int oi, double v, int i) {
    const bool on = ov != ov, vn = v != v;
    const bool gt = on ? !vn : ov > v;
    const bool eq = on ? vn : ov == v;
    return gt || (eq && oi < i);
}

}  // namespace fsnap
