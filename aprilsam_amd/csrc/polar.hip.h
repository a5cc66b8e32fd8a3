// polar.hip.h -- part of solver.hip.cpp (included after robust.hip.h).  Range, bearing and range-bearing factors.
//
// A packed polar factor occupies the ordinary slot of a binary factor in d_z / d_W.  Its measurement lives in a table of its own
// (GraphPack::pl_*, SoA):
//   pf[p]      packed entry of polar factor p
//   pkind[p]   RANGE / BEARING / RANGE_BEARING
//   pz[2p]     the measurement (one or two entries used)
//   pW[4p]     its information matrix (RANGE / BEARING: entry 0; RANGE_BEARING: 2 x 2 row-major)
// k_polar_slot writes the point-dependent xyt slot (z_eff, W_eff: polar.h) before k_linearize_t reads it, so the linearisation kernel (and
// its VGPR budget), assembly, factorisation and solves stay as they are; k_chi2_polar replaces the polar factors' terms of
// k_chi2 / k_lm_cost before the sums (one term under both conventions).  The formulas are polar.h's, shared with the host.  One thread per polar factor, plain loads and
// stores, no flags.
#pragma once
#include "polar.h"

namespace asam {

// q = position of b in a's frame and zh2 = the relative heading, at pts: the expressions of factor_residual (what k_linearize_t subtracts
// from the slot's z)
__device__ __forceinline__ void polar_q(const double *__restrict__ pts, int a, int b, double *q0, double *q1, double *zh2) {
    const double xa = pts[(size_t)3 * a], ya = pts[(size_t)3 * a + 1], ta = pts[(size_t)3 * a + 2];
    const double xb = pts[(size_t)3 * b], yb = pts[(size_t)3 * b + 1], tb = pts[(size_t)3 * b + 2];
    double sa, ca;
    sincos(ta, &sa, &ca);
    const double dx = xb - xa, dy = yb - ya;
    *q0 = ca * dx + sa * dy; *q1 = -sa * dx + ca * dy; *zh2 = tb - ta;
}

// one thread per polar factor: z_eff, W_eff at the l_points of a and b -> the factor's slot of Z / Wm
__global__ void __launch_bounds__(TPB) k_polar_slot(int P, const int *__restrict__ pf, const int *__restrict__ pkind, const double *__restrict__ pz,
                                                    const double *__restrict__ pW, const int *__restrict__ fa, const int *__restrict__ fb,
                                                    const double *__restrict__ lp, double *__restrict__ Z, double *__restrict__ Wm) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int f = pf[p], a = fa[f], b = fb[f];
    const double z[2] = { pz[(size_t)2 * p], pz[(size_t)2 * p + 1] };
    double w[4], q0, q1, zh2, ze[3], we[9];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = pW[(size_t)4 * p + i];
    polar_q(lp, a, b, &q0, &q1, &zh2);
    polar_slot(pkind[p], z, w, q0, q1, zh2, ze, we);
#pragma unroll
    for (int i = 0; i < 3; i++) Z[(size_t)3 * f + i] = ze[i];
#pragma unroll
    for (int i = 0; i < 9; i++) Wm[(size_t)9 * f + i] = we[i];
}

// one thread per polar factor: r_p' Wp r_p at st -> out[pf[p]] (april_graph_chi2: the full term, the rule of every type but xyt; the LM
// objective counts the same term, so both conventions launch this kernel, LM at the state array it is evaluating)
__global__ void __launch_bounds__(TPB) k_chi2_polar(int P, const int *__restrict__ pf, const int *__restrict__ pkind, const double *__restrict__ pz,
                                                    const double *__restrict__ pW, const int *__restrict__ fa, const int *__restrict__ fb,
                                                    const double *__restrict__ st, double *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int f = pf[p];
    const double z[2] = { pz[(size_t)2 * p], pz[(size_t)2 * p + 1] };
    double w[4], q0, q1, zh2;
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = pW[(size_t)4 * p + i];
    polar_q(st, fa[f], fb[f], &q0, &q1, &zh2);
    out[f] = polar_cost(pkind[p], z, w, q0, q1);
}

}  // namespace asam
