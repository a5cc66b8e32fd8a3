// robust.hip.h -- part of solver.hip.cpp (included after kernels.hip.h and maxmix.hip.h, whose factor_residual / rtWr it uses).  Robust
// losses on xyt / xytpos factors, iteratively reweighted least squares.
//
// A packed robust factor occupies its ordinary slot of d_z / d_W.  Its loss lives in a table of its own (GraphPack::rb_*, SoA):
//   rf[q]              packed entry of robust factor q
//   rkind[q], rc[q]    loss kind and scale c
//   rW0[9q]            the factor's unweighted W
//   rw[q]              the weight its most recent linearisation used
// k_robust_weight writes W_eff = w(s) W0 into the factor's slot before k_linearize_t reads it, so the linearisation kernel (and its VGPR
// budget) stays as it is; k_chi2_robust and k_lm_cost_robust replace the robust factors' terms of k_chi2 / k_lm_cost before the sums.
// The weighting and the term are written once, loss_weight_body and loss_term_body, over a loss policy that gives weight(s) and rho(s):
// RobustLoss here, GncLoss for the candidates of a GNC run (gnc.hip.h).  The formulas are robust.h's, shared with the host.  One thread
// per table row, plain loads and stores, no flags.  (The bodies take plain pointers: the wrappers' __restrict__ carries through the inlining.)
#pragma once
#include "robust.h"

namespace asam {

// residual of packed factor p at its points and s = r^T W0 r (k_chi2's expression); unary factors: pa only
__device__ __forceinline__ double robust_s(int p, int a, int b, const double *__restrict__ Z, const double *w0, const double *srca,
                                           const double *__restrict__ pts) {
    double z[3], pa[3], pb[3] = { 0, 0, 0 }, J0[9], J1[9], r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { z[k] = Z[(size_t)3 * p + k]; pa[k] = srca[k]; }
    if (b >= 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) pb[k] = pts[(size_t)3 * b + k];
    }
    factor_residual(b >= 0, pa, pb, z, J0, J1, r);
    return rtWr(w0, r);
}

// the loss of robust factor q: its own kind and scale, read from the table
struct RobustLoss {
    const int *kind; const double *c; int q;
    __device__ __forceinline__ double weight(double s) const { return robust_weight(kind[q], c[q], s); }
    __device__ __forceinline__ double rho(double s) const { return robust_rho(kind[q], c[q], s); }
};

// Row q of a loss table (packed entry tf[q], unweighted W tW0[9q]): w(s) at the point the linearisation that follows reads (xyt: lp;
// xytpos: upt when given, else st -- k_linearize_t's rule) -> W_eff = w * W0 into the factor's slot of Wm (one multiply per entry), w -> tw
template <class Loss>
__device__ __forceinline__ void loss_weight_body(int q, const int *tf, const double *tW0, const Loss &loss, const int *fa, const int *fb,
                                                 const double *Z, const double *lp, const double *st, const double *upt, double *Wm, double *tw) {
    const int p = tf[q], a = fa[p], b = fb[p];
    double w0[9];
#pragma unroll
    for (int i = 0; i < 9; i++) w0[i] = tW0[(size_t)9 * q + i];
    const double *srca = b >= 0 ? lp + (size_t)3 * a : (upt ? upt + (size_t)3 * p : st + (size_t)3 * a);
    const double w = loss.weight(robust_s(p, a, b, Z, w0, srca, lp));
#pragma unroll
    for (int i = 0; i < 9; i++) Wm[(size_t)9 * p + i] = w * w0[i];
    tw[q] = w;
}
// ... and its term of the objective at st: rho(r^T W0 r) -> out[tf[q]]; HALF_BINARY: 0.5 rho for xyt (k_chi2's convention)
template <bool HALF_BINARY, class Loss>
__device__ __forceinline__ void loss_term_body(int q, const int *tf, const double *tW0, const Loss &loss, const int *fa, const int *fb,
                                               const double *Z, const double *st, double *out) {
    const int p = tf[q], a = fa[p], b = fb[p];
    double w0[9];
#pragma unroll
    for (int i = 0; i < 9; i++) w0[i] = tW0[(size_t)9 * q + i];
    const double rho = loss.rho(robust_s(p, a, b, Z, w0, st + (size_t)3 * a, st));
    out[p] = (HALF_BINARY && b >= 0) ? 0.5 * rho : rho;
}

// one thread per robust factor: W_eff into its slot before the linearisation
__global__ void __launch_bounds__(TPB) k_robust_weight(int R, const int *__restrict__ rf, const int *__restrict__ rkind, const double *__restrict__ rc,
                                                       const double *__restrict__ rW0, const int *__restrict__ fa, const int *__restrict__ fb,
                                                       const double *__restrict__ Z, const double *__restrict__ lp, const double *__restrict__ st,
                                                       const double *__restrict__ upt, double *__restrict__ Wm, double *__restrict__ rw) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < R) loss_weight_body(q, rf, rW0, RobustLoss{ rkind, rc, q }, fa, fb, Z, lp, st, upt, Wm, rw);
}

// one thread per robust factor: its chi^2 term at st (0.5 rho(s) for xyt, rho(s) for xytpos) -> out[rf[q]]
__global__ void __launch_bounds__(TPB) k_chi2_robust(int R, const int *__restrict__ rf, const int *__restrict__ rkind, const double *__restrict__ rc,
                                                     const double *__restrict__ rW0, const int *__restrict__ fa, const int *__restrict__ fb,
                                                     const double *__restrict__ Z, const double *__restrict__ st, double *__restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < R) loss_term_body<true>(q, rf, rW0, RobustLoss{ rkind, rc, q }, fa, fb, Z, st, out);
}

// ... and its LM objective term, rho(s) for both types -> out[rf[q]]
__global__ void __launch_bounds__(TPB) k_lm_cost_robust(int R, const int *__restrict__ rf, const int *__restrict__ rkind, const double *__restrict__ rc,
                                                        const double *__restrict__ rW0, const int *__restrict__ fa, const int *__restrict__ fb,
                                                        const double *__restrict__ Z, const double *__restrict__ st, double *__restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < R) loss_term_body<false>(q, rf, rW0, RobustLoss{ rkind, rc, q }, fa, fb, Z, st, out);
}

}  // namespace asam
