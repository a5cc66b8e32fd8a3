// maxmix.hip.h -- part of solver.hip.cpp (included after kernels.hip.h, whose factor_residual / rtWr it uses).  Max-mixture factors.
//
// A packed max factor occupies an ordinary xyt slot of d_z / d_W.  Its components live in a table of their own (GraphPack::mx_*, SoA):
//   mf[m]                  packed entry of max factor m
//   mk[m] .. mk[m + 1]     its components
//   mz[3k], mW[9k], mc[k]  z, W and c = -2 logw - ln det W of component k (c formed on the host, in double)
// k_select_mixture writes the selected component's z / W into the factor's slot before k_linearize_t reads it, so the linearisation
// kernel (and its VGPR budget) stays as it is; k_chi2_mixture / k_lm_cost_mixture replace the max factors' terms of k_chi2 / k_lm_cost
// before the sums.  All three keep their own last lines of mixture_best, which restates host_objects.cpp: max_select -- score r^T W r + c,
// lowest index on a tie or a NaN.
#pragma once

namespace asam {

// the component of max factor m selected at `pts`: its index k, its score s = q + c_k and its q = r_k^T W_k r_k; p = the factor's packed entry
struct MixtureBest { int p, k0, k; double s, q; };
__device__ __forceinline__ MixtureBest mixture_best(int m, const int *mf, const int *mk, const double *mz, const double *mW, const double *mc,
                                                    const int *fa, const int *fb, const double *pts) {
    const int p = mf[m], k0 = mk[m], k1 = mk[m + 1];
    const int a = fa[p], b = fb[p];
    double pa[3], pb[3], J0[9], J1[9];
#pragma unroll
    for (int k = 0; k < 3; k++) { pa[k] = pts[(size_t)3 * a + k]; pb[k] = pts[(size_t)3 * b + k]; }
    MixtureBest best{ p, k0, k0, 0, 0 };
    for (int k = k0; k < k1; k++) {
        double z[3], w[9], r[3];
#pragma unroll
        for (int i = 0; i < 3; i++) z[i] = mz[(size_t)3 * k + i];
#pragma unroll
        for (int i = 0; i < 9; i++) w[i] = mW[(size_t)9 * k + i];
        factor_residual(true, pa, pb, z, J0, J1, r);
        const double q = rtWr(w, r), s = q + mc[k];
        if (k == k0 || s < best.s) { best.k = k; best.s = s; best.q = q; }
    }
    return best;
}

// one thread per max factor: the component selected at the factor's linearisation point -> its slot of Z / Wm, its index -> sel
__global__ void __launch_bounds__(TPB) k_select_mixture(int M, const int *__restrict__ mf, const int *__restrict__ mk, const double *__restrict__ mz,
                                                        const double *__restrict__ mW, const double *__restrict__ mc, const int *__restrict__ fa,
                                                        const int *__restrict__ fb, const double *__restrict__ lp, double *__restrict__ Z,
                                                        double *__restrict__ Wm, int *__restrict__ sel) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const MixtureBest best = mixture_best(m, mf, mk, mz, mW, mc, fa, fb, lp);
#pragma unroll
    for (int i = 0; i < 3; i++) Z[(size_t)3 * best.p + i] = mz[(size_t)3 * best.k + i];
#pragma unroll
    for (int i = 0; i < 9; i++) Wm[(size_t)9 * best.p + i] = mW[(size_t)9 * best.k + i];
    sel[m] = best.k - best.k0;
}

// one thread per max factor: its chi^2 term at `st` (0.5 r^T W r of the component selected there, k_chi2's expression) -> out[mf[m]]
__global__ void __launch_bounds__(TPB) k_chi2_mixture(int M, const int *__restrict__ mf, const int *__restrict__ mk, const double *__restrict__ mz,
                                                      const double *__restrict__ mW, const double *__restrict__ mc, const int *__restrict__ fa,
                                                      const int *__restrict__ fb, const double *__restrict__ st, double *__restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const MixtureBest best = mixture_best(m, mf, mk, mz, mW, mc, fa, fb, st);
    out[best.p] = 0.5 * best.q;
}

// ... and its LM objective term: min_k (r_k^T W_k r_k + c_k) at st, the score the selection minimises -> out[mf[m]]
__global__ void __launch_bounds__(TPB) k_lm_cost_mixture(int M, const int *__restrict__ mf, const int *__restrict__ mk, const double *__restrict__ mz,
                                                         const double *__restrict__ mW, const double *__restrict__ mc, const int *__restrict__ fa,
                                                         const int *__restrict__ fb, const double *__restrict__ st, double *__restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const MixtureBest best = mixture_best(m, mf, mk, mz, mW, mc, fa, fb, st);
    out[best.p] = best.s;
}

}  // namespace asam
