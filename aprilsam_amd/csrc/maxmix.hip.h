// maxmix.hip.h -- part of solver.hip.cpp (included after kernels.hip.h, whose factor_residual / rtWr it uses).  Max-mixture factors.
//
// A packed max factor occupies an ordinary xyt slot of d_z / d_W.  Its components live in a table of their own (GraphPack::mx_*, SoA):
//   mf[m]                  packed entry of max factor m
//   mk[m] .. mk[m + 1]     its components
//   mz[3k], mW[9k], mc[k]  z, W and c = -2 logw - ln det W of component k (c formed on the host, in double)
// k_select_mixture writes the selected component's z / W into the factor's slot before k_linearize_t reads it, so the linearisation
// kernel (and its VGPR budget) stays as it is; k_chi2_mixture replaces the max factors' terms of k_chi2's output before the sums.
// Both restate host_objects.cpp: max_select -- score r^T W r + c, lowest index on a tie or a NaN.
#pragma once

namespace asam {

// one thread per max factor: the component selected at the factor's linearisation point -> its slot of Z / Wm, its index -> sel
__global__ void __launch_bounds__(TPB) k_select_mixture(int M, const int *__restrict__ mf, const int *__restrict__ mk, const double *__restrict__ mz,
                                                        const double *__restrict__ mW, const double *__restrict__ mc, const int *__restrict__ fa,
                                                        const int *__restrict__ fb, const double *__restrict__ lp, double *__restrict__ Z,
                                                        double *__restrict__ Wm, int *__restrict__ sel) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int p = mf[m], k0 = mk[m], k1 = mk[m + 1];
    const int a = fa[p], b = fb[p];
    double pa[3], pb[3], J0[9], J1[9];
#pragma unroll
    for (int k = 0; k < 3; k++) { pa[k] = lp[(size_t)3 * a + k]; pb[k] = lp[(size_t)3 * b + k]; }
    int best = k0; double sbest = 0;
    for (int k = k0; k < k1; k++) {
        double z[3], w[9], r[3];
#pragma unroll
        for (int i = 0; i < 3; i++) z[i] = mz[(size_t)3 * k + i];
#pragma unroll
        for (int i = 0; i < 9; i++) w[i] = mW[(size_t)9 * k + i];
        factor_residual(true, pa, pb, z, J0, J1, r);
        const double s = rtWr(w, r) + mc[k];
        if (k == k0) sbest = s;
        else if (s < sbest) { best = k; sbest = s; }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) Z[(size_t)3 * p + i] = mz[(size_t)3 * best + i];
#pragma unroll
    for (int i = 0; i < 9; i++) Wm[(size_t)9 * p + i] = mW[(size_t)9 * best + i];
    sel[m] = best - k0;
}

// one thread per max factor: its chi^2 term at `st` (0.5 r^T W r of the component selected there, k_chi2's expression) -> out[mf[m]]
__global__ void __launch_bounds__(TPB) k_chi2_mixture(int M, const int *__restrict__ mf, const int *__restrict__ mk, const double *__restrict__ mz,
                                                      const double *__restrict__ mW, const double *__restrict__ mc, const int *__restrict__ fa,
                                                      const int *__restrict__ fb, const double *__restrict__ st, double *__restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int p = mf[m], k0 = mk[m], k1 = mk[m + 1];
    const int a = fa[p], b = fb[p];
    double pa[3], pb[3], J0[9], J1[9];
#pragma unroll
    for (int k = 0; k < 3; k++) { pa[k] = st[(size_t)3 * a + k]; pb[k] = st[(size_t)3 * b + k]; }
    double sbest = 0, qbest = 0;
    for (int k = k0; k < k1; k++) {
        double z[3], w[9], r[3];
#pragma unroll
        for (int i = 0; i < 3; i++) z[i] = mz[(size_t)3 * k + i];
#pragma unroll
        for (int i = 0; i < 9; i++) w[i] = mW[(size_t)9 * k + i];
        factor_residual(true, pa, pb, z, J0, J1, r);
        const double q = rtWr(w, r), s = q + mc[k];
        if (k == k0 || s < sbest) { sbest = s; qbest = q; }
    }
    out[p] = 0.5 * qbest;
}

}  // namespace asam
