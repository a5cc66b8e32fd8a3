// gnc.hip.h -- part of solver.hip.cpp (included after robust.hip.h, whose robust_s it uses).  Graduated non-convexity (DESIGN.md section
// 17): for the length of one aprilsam_amd_optimize_gnc call the candidate factors carry the surrogate loss of robust.h's gnc_weight /
// gnc_rho at the control parameter mu.
//
// A candidate occupies its ordinary slot of d_z / d_W.  The table (GraphPack::gc_*, device only, in the caller's order):
//   gf[i]      packed entry of candidate i
//   gW0[9i]    its plain W
//   gw[i]      the weight its most recent linearisation used
//   par        GncPar: loss, c and mu.  mu is READ FROM MEMORY by every kernel below, so that a captured LM iteration is the same graph
//              for every stage; k_gnc_set_mu (one thread, launched between stages, never captured) writes it
// k_gnc_weight writes W_eff = w_mu(s) W0 into the slot before k_linearize_t reads it and k_gnc_cost replaces the candidates' terms of
// k_lm_cost: the bodies k_robust_weight / k_lm_cost_robust run for a factor's own loss, with GncLoss for the policy.  One thread per
// candidate, plain loads and stores; the two reductions (largest s, any weight strictly between 0 and 1) are k_gnc_max / k_gnc_max_parts,
// the max op of the one reducer (kernels.hip.h).
#pragma once
#include "robust.h"

namespace asam {

struct GncPar { double mu, c; int loss, pad; };

__global__ void k_gnc_set_mu(GncPar *__restrict__ par, double mu) {
    if (blockIdx.x == 0 && threadIdx.x == 0) par->mu = mu;
}

// the surrogate at the run's current mu: loss_weight_body / loss_term_body's policy for a candidate (robust.hip.h)
struct GncLoss {
    const GncPar *par;
    __device__ __forceinline__ double weight(double s) const { return gnc_weight(par->loss, par->c, par->mu, s); }
    __device__ __forceinline__ double rho(double s) const { return gnc_rho(par->loss, par->c, par->mu, s); }
};

// W_eff = w_mu(s) W0 into the candidates' slots of Wm, w -> gw; s where k_robust_weight takes it
__global__ void __launch_bounds__(TPB) k_gnc_weight(int n, const int *__restrict__ gf, const double *__restrict__ gW0, const GncPar *__restrict__ par,
                                                    const int *__restrict__ fa, const int *__restrict__ fb, const double *__restrict__ Z,
                                                    const double *__restrict__ lp, const double *__restrict__ st, const double *__restrict__ upt,
                                                    double *__restrict__ Wm, double *__restrict__ gw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) loss_weight_body(i, gf, gW0, GncLoss{ par }, fa, fb, Z, lp, st, upt, Wm, gw);
}

// rho_mu(r^T W0 r) at st (the LM objective term; the chi^2 convention never counts the surrogate) -> out[gf[i]]
__global__ void __launch_bounds__(TPB) k_gnc_cost(int n, const int *__restrict__ gf, const double *__restrict__ gW0, const GncPar *__restrict__ par,
                                                  const int *__restrict__ fa, const int *__restrict__ fb, const double *__restrict__ Z,
                                                  const double *__restrict__ st, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) loss_term_body<false>(i, gf, gW0, GncLoss{ par }, fa, fb, Z, st, out);
}

// what = 0: s at st -> out[i] (the start: its maximum is s_max)
// what = 1: 1.0 if w_mu(s) at st lies strictly between 0 and 1 (or is NaN), else 0.0 -> out[i] (TLS: the maximum is the "not all binary" flag)
__global__ void __launch_bounds__(TPB) k_gnc_probe(int n, const int *__restrict__ gf, const double *__restrict__ gW0, const GncPar *__restrict__ par,
                                                   int what, const int *__restrict__ fa, const int *__restrict__ fb, const double *__restrict__ Z,
                                                   const double *__restrict__ st, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = gf[i], a = fa[p], b = fb[p];
    double w0[9];
#pragma unroll
    for (int k = 0; k < 9; k++) w0[k] = gW0[(size_t)9 * i + k];
    const double s = robust_s(p, a, b, Z, w0, st + (size_t)3 * a, st);
    if (what == 0) { out[i] = s; return; }
    const double w = gnc_weight(par->loss, par->c, par->mu, s);
    out[i] = (w == 0.0 || w == 1.0) ? 0.0 : 1.0;
}

// the end of the call: w_mu(s) at st -> out[i], inlier (s <= c^2) as 1.0 / 0.0 -> out[n + i], and the plain W back into the slot
__global__ void __launch_bounds__(TPB) k_gnc_final(int n, const int *__restrict__ gf, const double *__restrict__ gW0, const GncPar *__restrict__ par,
                                                   const int *__restrict__ fa, const int *__restrict__ fb, const double *__restrict__ Z,
                                                   const double *__restrict__ st, double *__restrict__ Wm, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = gf[i], a = fa[p], b = fb[p];
    double w0[9];
#pragma unroll
    for (int k = 0; k < 9; k++) w0[k] = gW0[(size_t)9 * i + k];
    const double c = par->c, s = robust_s(p, a, b, Z, w0, st + (size_t)3 * a, st);
    out[i] = gnc_weight(par->loss, c, par->mu, s);
    out[n + i] = s <= c * c ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) Wm[(size_t)9 * p + k] = w0[k];
}

}  // namespace asam
