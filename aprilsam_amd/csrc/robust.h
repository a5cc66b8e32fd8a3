// robust.h -- the robust losses of xyt / xytpos factors, shared by host_objects.cpp (host eval, the incremental
// path's weighting of new factors) and the HIP translation unit (robust.hip.h).  s = r^T W r is the squared Mahalanobis distance of the
// plain factor, c > 0 a threshold on sqrt(s).  The solver linearises the plain factor with W_eff = w(s) W (IRLS); the objective term is
// rho(s).  Every branch is written so that a NaN s gives a NaN weight and a NaN rho: a robust factor that goes non-finite fails the call
// as a plain one does.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define ROBUST_HD __host__ __device__
#else
#define ROBUST_HD
#endif

namespace asam {

enum { ROBUST_NONE = 0, ROBUST_HUBER = 1, ROBUST_CAUCHY = 2, ROBUST_DCS = 3 };

// w(s) = rho'(s); kind NONE (never packed as robust) gives 1
inline ROBUST_HD double robust_weight(int kind, double c, double s) {
    const double cc = c * c;
    switch (kind) {
    case ROBUST_HUBER: return s <= cc ? 1.0 : c / sqrt(s);
    case ROBUST_CAUCHY: return 1.0 / (1.0 + s / cc);
    case ROBUST_DCS: { const double t = s + cc; return s <= cc ? 1.0 : 4.0 * cc * cc / (t * t); }
    default: return 1.0;
    }
}
// rho(s); NONE: s
inline ROBUST_HD double robust_rho(int kind, double c, double s) {
    const double cc = c * c;
    switch (kind) {
    case ROBUST_HUBER: return s <= cc ? s : 2.0 * c * sqrt(s) - cc;
    case ROBUST_CAUCHY: return cc * log1p(s / cc);
    case ROBUST_DCS: return s <= cc ? s : cc * (3.0 * s - cc) / (s + cc);
    default: return s;
    }
}
// Graduated non-convexity: the surrogate of Geman-McClure / truncated least squares at control parameter mu, never
// a factor's own loss (set_robust refuses the kinds) -- aprilsam_amd_optimize_gnc applies it to its candidates for the length of the call.
// mu = +inf (TLS, every candidate an inlier at the start) is the limit, TLS itself: lo = hi = c^2.  A NaN s fails every comparison and
// goes through the sqrt: NaN weight, NaN rho.
enum { GNC_GM = 1, GNC_TLS = 2 };
inline ROBUST_HD double gnc_weight(int loss, double c, double mu, double s) {
    const double cc = c * c;
    if (loss == GNC_GM) { const double m = mu * cc, q = m / (m + s); return q * q; }
    const bool lim = mu > 1.7976931348623157e308;
    const double lo = lim ? cc : mu / (mu + 1.0) * cc, hi = lim ? cc : (mu + 1.0) / mu * cc;
    if (s <= lo) return 1.0;
    if (s >= hi) return 0.0;
    return c * sqrt(mu * (mu + 1.0) / s) - mu;
}
inline ROBUST_HD double gnc_rho(int loss, double c, double mu, double s) {
    const double cc = c * c;
    if (loss == GNC_GM) { const double m = mu * cc; return m * s / (m + s); }
    const bool lim = mu > 1.7976931348623157e308;
    const double lo = lim ? cc : mu / (mu + 1.0) * cc, hi = lim ? cc : (mu + 1.0) / mu * cc;
    if (s <= lo) return s;
    if (s >= hi) return cc;
    return 2.0 * c * sqrt(mu * (mu + 1.0) * s) - mu * (cc + s);
}
// the information matrix a robust factor may carry: bitwise symmetric, all three leading minors > 0
inline bool robust_spd(const double *w) {
    if (w[1] != w[3] || w[2] != w[6] || w[5] != w[7]) return false;
    const double m1 = w[0], m2 = w[0] * w[4] - w[1] * w[3];
    const double m3 = w[0] * (w[4] * w[8] - w[5] * w[7]) - w[1] * (w[3] * w[8] - w[5] * w[6]) + w[2] * (w[3] * w[7] - w[4] * w[6]);
    return m1 > 0 && m2 > 0 && m3 > 0;
}

}  // namespace asam
