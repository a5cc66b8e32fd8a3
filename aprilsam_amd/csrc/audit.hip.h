// audit.hip.h -- part of solver.hip.cpp (included after kernels.hip.h and selinv.hip.h, whose factor_residual / rtWr / a_v and
// sel_local_row it uses).  The per-factor audit: leverage and leave-one-out distance of the factors of the system
// the last solver call factorised, behind the selected inversion (selinv.hip.h).
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

// One listed factor per group of AUDIT_LANES = 8 consecutive lanes: the six columns of the factor's Sigma block (two 3-element pieces at
// stride R each) are spread over the group's lanes, every lane forms its column's share of P, and the nine sums are taken by shuffles.
// Plain loads and stores: no LDS, no atomics, no flags.  Measured against one thread per factor (the same code with a group of one,
// profiles/factor_audit.txt): 0.262 against 0.282 ms for the 397 531 factors of the 10^5 lattice, 2.43 against 2.50 ms at 10^6.
//   list[i]     the factor's packed entry (GraphPack::g2p), -1: not auditable -> four NaN
//   fmask       null, or per listed factor bit 0 = node a was fixed in the factorised system, bit 1 = node b (fixed_query_mask): the rows
//               and columns of a fixed node are exact zeros before P is formed, as k_fix_cov makes them
//   fa fb Z Wm  the linearisation slots as the factorised system saw them (robust weight applied, max-mixture component selected, a polar
//               measurement in its xyt form); b < 0: xytpos prior, J = I
//   lp, dx      the linearisation points and the step of that system, in node order; upt: null, or per packed entry the point a prior
//               was linearised at (an incremental call that fell back to a batch step)
//   pos ... sig the Sigma pool and its tables, read as k_marginal_extract reads them: the front of the earlier-eliminated node, the
//               other node's rows by sel_local_row
// With J = [J_a J_b] and r from factor_residual at lp:  v = r - J (dx_a, dx_b)  (k_lm_model's residual, its sign),  P = J Sigma_ff J',
// M = I - P W.  out[4 i ..] = v' W v,  tr(P W),  v' W M^-1 v,  det M.  det by cofactors, the solve by the adjugate, no pivot threshold:
// only det <= 0 or not finite gives a NaN distance.
// (the one-thread form the comparison was taken against is this code with a group of one: compile solver.hip.cpp with
// -DAPRILSAM_AMD_AUDIT_LANES=1 into a library of its own and hand it to tools/audit_time.py --lib; profiles/README.md has the commands)
#ifndef APRILSAM_AMD_AUDIT_LANES
#define APRILSAM_AMD_AUDIT_LANES 8
#endif
constexpr int AUDIT_LANES = APRILSAM_AMD_AUDIT_LANES;
__global__ void __launch_bounds__(256) k_factor_audit(int n, const int *__restrict__ list, const int *__restrict__ fmask, const int *__restrict__ fa,
                                                      const int *__restrict__ fb, const double *__restrict__ Z, const double *__restrict__ Wm,
                                                      const double *__restrict__ lp, const double *__restrict__ dx, const double *__restrict__ upt,
                                                      const int *__restrict__ pos, const int *__restrict__ pos_front, const SelFront *__restrict__ fr,
                                                      const int *__restrict__ rows, const double *__restrict__ sig, double *__restrict__ out) {
    constexpr int G = AUDIT_LANES;
    static_assert(256 % G == 0 && (G & (G - 1)) == 0, "whole groups per workgroup, a power of two for the shuffles");
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = g / G;
    const int sub = (int)(g % G);
    if (i >= n) return;                                     // (whole groups leave together: 256 is a multiple of G)
    double *o = out + 4 * i;
    const double qnan = __builtin_nan("");
    auto refuse = [&]() { if (sub == 0) { o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = qnan; } };
    const int p = list[i];
    if (p < 0) { refuse(); return; }
    const int a = fa[p], b = fb[p];
    if (a < 0) { refuse(); return; }
    const bool binary = b >= 0;
    double w[9], z[3], J0[9], J1[9], r[3], pa[3], pb[3] = { 0, 0, 0 }, ha[3], hb[3] = { 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 9; k++) w[k] = Wm[(size_t)9 * p + k];
    const double *src = (!binary && upt) ? upt + (size_t)3 * p : lp + (size_t)3 * a;
#pragma unroll
    for (int k = 0; k < 3; k++) { z[k] = Z[(size_t)3 * p + k]; pa[k] = src[k]; ha[k] = dx[(size_t)3 * a + k]; }
    if (binary) {
#pragma unroll
        for (int k = 0; k < 3; k++) { pb[k] = lp[(size_t)3 * b + k]; hb[k] = dx[(size_t)3 * b + k]; }
    }
    factor_residual(binary, pa, pb, z, J0, J1, r);
    double v[3];
    if (binary) {
        double d0[3], d1[3];
        a_v(J0, ha, d0); a_v(J1, hb, d1);
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = r[k] - (d0[k] + d1[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = r[k] - ha[k];
    }
    const int qa = pos[a], qb = binary ? pos[b] : qa;
    const SelFront F = fr[pos_front[min(qa, qb)]];
    const int la = sel_local_row(F, rows, qa), lb = binary ? sel_local_row(F, rows, qb) : la;
    if (la < 0 || lb < 0) { refuse(); return; }             // (never for a factor of the factorised system: its pair is on the pattern of L)
    const int m = fmask ? fmask[i] : 0;
    // P = J Sigma_ff J' column by column of Sigma_ff: u = J Sigma_ff[:, c], P += u (J[:, c])'
    double P[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const int nc = binary ? 6 : 3;
    for (int c = sub; c < nc; c += G) {
        const bool cb = c >= 3;
        if (m & (cb ? 2 : 1)) continue;
        const double *col = sig + F.off + (long long)((cb ? lb : la) + c % 3) * F.R;
        double sa[3], u[3];
#pragma unroll
        for (int k = 0; k < 3; k++) sa[k] = (m & 1) ? 0.0 : col[la + k];
        if (binary) {
            double sb[3], u0[3], u1[3];
#pragma unroll
            for (int k = 0; k < 3; k++) sb[k] = (m & 2) ? 0.0 : col[lb + k];
            a_v(J0, sa, u0); a_v(J1, sb, u1);
#pragma unroll
            for (int k = 0; k < 3; k++) u[k] = u0[k] + u1[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) u[k] = sa[k];
        }
        const double *Jc = cb ? J1 : J0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double jc = Jc[3 * k + c % 3];
#pragma unroll
            for (int e = 0; e < 3; e++) P[3 * e + k] += u[e] * jc;
        }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1)
#pragma unroll
        for (int e = 0; e < 9; e++) P[e] += __shfl_xor(P[e], off, G);
    if (sub != 0) return;
    double M[9], lev = 0;
#pragma unroll
    for (int e = 0; e < 3; e++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double pw = P[3 * e] * w[k] + P[3 * e + 1] * w[3 + k] + P[3 * e + 2] * w[6 + k];
            if (e == k) lev += pw;
            M[3 * e + k] = (e == k ? 1.0 : 0.0) - pw;
        }
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
    double Wv[3];
    a_v(w, v, Wv);
    const double chi2 = v[0] * Wv[0] + v[1] * Wv[1] + v[2] * Wv[2];
    double d2 = qnan;
    if (det > 0 && isfinite(det)) {
        const double x0 = c00 * v[0] + (M[2] * M[7] - M[1] * M[8]) * v[1] + (M[1] * M[5] - M[2] * M[4]) * v[2];
        const double x1 = c01 * v[0] + (M[0] * M[8] - M[2] * M[6]) * v[1] + (M[2] * M[3] - M[0] * M[5]) * v[2];
        const double x2 = c02 * v[0] + (M[1] * M[6] - M[0] * M[7]) * v[1] + (M[0] * M[4] - M[1] * M[3]) * v[2];
        d2 = (Wv[0] * x0 + Wv[1] * x1 + Wv[2] * x2) / det;
    }
    o[0] = chi2; o[1] = lev; o[2] = d2; o[3] = det;
}

}  // namespace asam
