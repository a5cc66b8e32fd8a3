// polar.h -- range, bearing and range-bearing factors, shared by host_objects.cpp (host eval, the incremental path's
// slots of new factors, aprilsam_amd_debug_polar_slot) and the HIP translation unit (polar.hip.h).  Header-only: the sanitised host build
// compiles it with the host sources.
//
// `a` observes `b`.  q = (zh0, zh1) is the position of b in a's frame, exactly what an xyt factor predicts (factor_residual), zh2 the
// relative heading it predicts.  rho = |q|, beta = atan2(q1, q0):
//   RANGE          h = rho            z = {rho}        Wp = {w}
//   BEARING        h = beta           z = {beta}       Wp = {w}
//   RANGE_BEARING  h = (rho, beta)    z = {rho, beta}  Wp 2 x 2 row-major
// r_p = z - h(q), the bearing component wrapped with mod2pi.  With G = dh/dq (m x 2) the factor's Gauss-Newton contribution is that of an
// xyt factor whose slot holds
//   W_eff = [[G' Wp G, 0], [0, 0]]      r_eff = G' (G G')^-1 r_p      z_eff = (q + r_eff, zh2)
// (J_xyt' W_eff J_xyt = J_p' Wp J_p and J_xyt' W_eff (z_eff - zh) = J_p' Wp r_p: G G' (G G')^-1 = I).  The rows of G are orthogonal --
// G G' = diag(1, 1 / rho^2) -- so no 2 x 2 solve appears.  rho^2 == 0: G does not exist; W_eff = 0 and z_eff = (q, zh2), the factor is
// silent for that linearisation.  No threshold: a tiny non-zero rho keeps its 1 / rho Jacobian.  A non-finite input propagates.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define POLAR_HD __host__ __device__
#else
#define POLAR_HD
#endif

namespace asam {

enum { POLAR_RANGE = 1, POLAR_BEARING = 2, POLAR_RANGE_BEARING = 3 };

inline POLAR_HD int polar_rows(int kind) { return kind == POLAR_RANGE_BEARING ? 2 : 1; }

inline POLAR_HD double polar_mod2pi(double v) {            // math_util.h:113-122, range [-pi, pi)
    const double TWOPI = 6.2831853071795862319959, PI_ = 3.141592653589793238462643383279502884196;
    const double vin = v + PI_;
    return (vin - TWOPI * floor(vin / TWOPI)) - PI_;
}

// r_p = z - h(q) (m = polar_rows(kind) entries of r are written)
inline POLAR_HD void polar_residual(int kind, const double *z, double q0, double q1, double *r) {
    if (kind == POLAR_RANGE) r[0] = z[0] - sqrt(q0 * q0 + q1 * q1);
    else if (kind == POLAR_BEARING) r[0] = polar_mod2pi(z[0] - atan2(q1, q0));
    else { r[0] = z[0] - sqrt(q0 * q0 + q1 * q1); r[1] = polar_mod2pi(z[1] - atan2(q1, q0)); }
}

// G = dh/dq, m x 2 row-major; false (G untouched) when rho^2 == 0
inline POLAR_HD bool polar_G(int kind, double q0, double q1, double *G) {
    const double rho2 = q0 * q0 + q1 * q1;
    if (rho2 == 0) return false;
    const double rho = sqrt(rho2);
    int k = 0;
    if (kind != POLAR_BEARING) { G[0] = q0 / rho; G[1] = q1 / rho; k = 2; }
    if (kind != POLAR_RANGE) { G[k] = -q1 / rho2; G[k + 1] = q0 / rho2; }
    return true;
}

// r_p' Wp r_p; Wp: m x m row-major (the association of eval_finish, one row of Wp at a time)
inline POLAR_HD double polar_cost(int kind, const double *z, const double *Wp, double q0, double q1) {
    double r[2];
    polar_residual(kind, z, q0, q1, r);
    if (kind != POLAR_RANGE_BEARING) return r[0] * (Wp[0] * r[0]);
    const double X0 = Wp[0] * r[0] + Wp[1] * r[1], X1 = Wp[2] * r[0] + Wp[3] * r[1];
    return r[0] * X0 + r[1] * X1;
}

// the xyt slot at q (zh2: the relative heading the xyt factor predicts there): z_eff[3], W_eff[9] row-major.  W_eff's upper triangle is
// computed and mirrored: bitwise symmetric
inline POLAR_HD void polar_slot(int kind, const double *z, const double *Wp, double q0, double q1, double zh2, double *z_eff, double *W_eff) {
    for (int i = 0; i < 9; i++) W_eff[i] = 0;
    z_eff[0] = q0; z_eff[1] = q1; z_eff[2] = zh2;
    const double rho2 = q0 * q0 + q1 * q1;
    if (rho2 == 0) return;
    const double rho = sqrt(rho2);
    double r[2];
    polar_residual(kind, z, q0, q1, r);
    const double u0 = q0 / rho, u1 = q1 / rho;           // d rho / dq
    const double v0 = -q1 / rho2, v1 = q0 / rho2;        // d beta / dq
    double a00, a01, a11;
    if (kind == POLAR_RANGE) {
        const double w = Wp[0];
        a00 = w * (u0 * u0); a01 = w * (u0 * u1); a11 = w * (u1 * u1);
        z_eff[0] = q0 + u0 * r[0]; z_eff[1] = q1 + u1 * r[0];
    } else if (kind == POLAR_BEARING) {
        const double w = Wp[0];
        a00 = w * (v0 * v0); a01 = w * (v0 * v1); a11 = w * (v1 * v1);
        z_eff[0] = q0 + -q1 * r[0]; z_eff[1] = q1 + q0 * r[0];          // G' (G G')^-1 = rho^2 (v0, v1)' = (-q1, q0)'
    } else {
        const double w00 = Wp[0], w01 = Wp[1], w11 = Wp[3];
        a00 = w00 * (u0 * u0) + w01 * (2.0 * (u0 * v0)) + w11 * (v0 * v0);
        a01 = w00 * (u0 * u1) + w01 * (u0 * v1 + v0 * u1) + w11 * (v0 * v1);
        a11 = w00 * (u1 * u1) + w01 * (2.0 * (u1 * v1)) + w11 * (v1 * v1);
        z_eff[0] = q0 + (u0 * r[0] + -q1 * r[1]); z_eff[1] = q1 + (u1 * r[0] + q0 * r[1]);
    }
    W_eff[0] = a00; W_eff[1] = a01; W_eff[3] = a01; W_eff[4] = a11;
}

// host: q and zh2 at poses pa, pb (xyt_eval_at's expressions), then the slot
inline void polar_host_q(const double *pa, const double *pb, double *q0, double *q1, double *zh2) {
    const double ca = cos(pa[2]), sa = sin(pa[2]);
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    *q0 = ca * dx + sa * dy; *q1 = -sa * dx + ca * dy; *zh2 = pb[2] - pa[2];
}
inline void polar_host_slot(int kind, const double *z, const double *Wp, const double *pa, const double *pb, double *z_eff, double *W_eff) {
    double q0, q1, zh2;
    polar_host_q(pa, pb, &q0, &q1, &zh2);
    polar_slot(kind, z, Wp, q0, q1, zh2, z_eff, W_eff);
}

// the information matrix a polar factor may carry: finite, bitwise symmetric, positive definite (m x m)
inline bool polar_spd(int kind, const double *w) {
    if (kind != POLAR_RANGE_BEARING) return std::isfinite(w[0]) && w[0] > 0;
    for (int i = 0; i < 4; i++) if (!std::isfinite(w[i])) return false;
    return w[1] == w[2] && w[0] > 0 && w[0] * w[3] - w[1] * w[2] > 0;
}

// ---- gating of a candidate polar measurement -------------------------------------------------------------------
// The Mahalanobis test of the m-row innovation of a candidate (kind, z, Wp) between a and b at their states pa, pb, with C the 6 x 6 joint
// covariance of (a, b), a's unknowns first, row-major:
//   q, r      position of b in a's frame and r = z - h(q), the bearing row wrapped (polar_residual); the expressions of factor_residual
//   J_q       rows 0 and 1 of the xyt factor's [J_a J_b] (2 x 6; b's heading column is zero, so pb[2] and row / column 5 of C are never read)
//   J_p = G J_q,   S = J_p C J_p' + Wp^-1 (2 x 2: the adjugate; one row: 1 / w),   d2 = r' S^-1 r (a 2 x 2 Cholesky, or a division)
// S: m x m row-major, the upper triangle computed and mirrored.  rho^2 == 0: G does not exist -- false, d2 and the m x m entries of S NaN.
// No threshold, as for the slot.
inline POLAR_HD bool polar_gate(int kind, const double *z, const double *Wp, const double *pa, const double *pb, const double *C, double *d2, double *S) {
    const int m = polar_rows(kind);
    double sa, ca;
#ifdef __HIP_DEVICE_COMPILE__
    sincos(pa[2], &sa, &ca);
#else
    sa = sin(pa[2]); ca = cos(pa[2]);
#endif
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    const double q0 = ca * dx + sa * dy, q1 = -sa * dx + ca * dy;
    double G[4];
    if (!polar_G(kind, q0, q1, G)) {
        *d2 = NAN;
        for (int i = 0; i < m * m; i++) S[i] = NAN;
        return false;
    }
    double r[2];
    polar_residual(kind, z, q0, q1, r);
    const double Jq[10] = { -ca, -sa, -sa * dx + ca * dy, ca, sa,             // (column 5 is zero: left out)
                            sa, -ca, -ca * dx - sa * dy, -sa, ca };
    double Jp[10], JC[10];                                                    // m x 5
    for (int i = 0; i < m; i++)
        for (int k = 0; k < 5; k++) Jp[5 * i + k] = G[2 * i] * Jq[k] + G[2 * i + 1] * Jq[5 + k];
    for (int i = 0; i < m; i++)
        for (int j = 0; j < 5; j++) {
            double v = 0.0;
            for (int k = 0; k < 5; k++) v += Jp[5 * i + k] * C[6 * k + j];
            JC[5 * i + j] = v;
        }
    double P[3] = { 0.0, 0.0, 0.0 };                                          // J_p C J_p': (0,0), (0,1), (1,1)
    for (int k = 0; k < 5; k++) P[0] += JC[k] * Jp[k];
    if (m == 1) {
        const double s = P[0] + 1.0 / Wp[0];
        S[0] = s;
        *d2 = r[0] * r[0] / s;
        return true;
    }
    for (int k = 0; k < 5; k++) { P[1] += JC[k] * Jp[5 + k]; P[2] += JC[5 + k] * Jp[5 + k]; }
    const double det = Wp[0] * Wp[3] - Wp[1] * Wp[2];
    const double s00 = P[0] + Wp[3] / det, s01 = P[1] + -Wp[1] / det, s11 = P[2] + Wp[0] / det;
    S[0] = s00; S[1] = s01; S[2] = s01; S[3] = s11;
    const double l00 = sqrt(s00), l10 = s01 / l00, l11 = sqrt(s11 - l10 * l10);
    const double y0 = r[0] / l00, y1 = (r[1] - l10 * y0) / l11;
    *d2 = y0 * y0 + y1 * y1;
    return true;
}

// host: what aprilsam_amd_gate_polar and aprilsam_amd_associate_polar can judge of n measurements (kind[i], z[2 i..], W[4 i..]) without a
// graph or a device: 0, or the refusal's code with its reason in *why.  Only the entries a kind reads are looked at: z[2 i] and W[4 i] for
// one row, all of both for two.
inline int polar_gate_args(int n, const int *kind, const double *z, const double *W, const char **why) {
    for (int i = 0; i < n; i++) {
        if (kind[i] < POLAR_RANGE || kind[i] > POLAR_RANGE_BEARING) { *why = "a kind outside RANGE, BEARING, RANGE_BEARING"; return -13; }
        const int m = polar_rows(kind[i]);
        for (int k = 0; k < m; k++) if (!std::isfinite(z[2 * i + k])) { *why = "a non-finite measurement"; return -13; }
        for (int k = 0; k < m * m; k++) if (!std::isfinite(W[4 * i + k])) { *why = "a non-finite information matrix"; return -13; }
    }
    for (int i = 0; i < n; i++)
        if (!polar_spd(kind[i], W + 4 * i)) { *why = "an information matrix that is not symmetric positive definite"; return -12; }
    return 0;
}

}  // namespace asam
