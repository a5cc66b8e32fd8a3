// fixed.hip.h -- part of solver.hip.cpp (included after polar.hip.h).  Fixed nodes: poses held constant.
//
// A fixed node keeps its place in the elimination order; what makes it constant is a mask over the contribution slots of d_H plus one
// entry of d_lambda, applied after everything that fills the slots of a linearisation and before the first assembly kernel reads them.
// The pack keeps a table (GraphPack::fx_*):
//   fnode[i]   id of fixed node i
//   rec[r]     .x = a packed entry with a fixed endpoint, .y = which of its five slots are zeroed:
//              bit 0 (a,a) block   bit 1 off-diagonal block   bit 2 (b,b) block   bit 3 rhs of a   bit 4 rhs of b
// The slot NUMBERS belong to the plan (slot_blk / slot_rhs, one plan per param) and one graph may be driven by several params, so a
// record names the entry and the kernel looks the numbers up where k_linearize_t does.  k_fix_cov makes the blocks of fixed nodes exact
// zeros in the covariances that aprilsam_amd_marginals* and aprilsam_amd_gate_xyt hand out.  One thread per record / node / query, plain
// loads and vector stores, no LDS, no atomics, no flags.
#pragma once

namespace asam {

constexpr int FX_AA = 1, FX_AB = 2, FX_BB = 4, FX_GA = 8, FX_GB = 16;

// threads [0, R): record r -- the listed slots of Hc become +0 (a rhs slot is 9 doubles wide and only its first three are used);
// threads [R, R + NF): fixed node i -- lambda at its elimination position becomes 1.0: with every contribution to its diagonal block
// zeroed, the assembled block is exactly 1.0 * I whatever tikhanov or LM's damping is
__global__ void __launch_bounds__(TPB) k_fix_mask(int R, const int2 *__restrict__ rec, int NF, const int *__restrict__ fnode, const int *__restrict__ pos,
                                                  const int *__restrict__ slot_blk, const int *__restrict__ slot_rhs, double *__restrict__ Hc,
                                                  double *__restrict__ lambda) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R) {
        if (t - R < NF) lambda[pos[fnode[t - R]]] = 1.0;
        return;
    }
    const int f = rec[t].x, m = rec[t].y;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int sl = (m >> k) & 1 ? slot_blk[3 * f + k] : -1;
        if (sl < 0) continue;
        double *o = Hc + (size_t)sl * 9;
#pragma unroll
        for (int i = 0; i < 9; i++) o[i] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int sl = (m >> (3 + k)) & 1 ? slot_rhs[2 * f + k] : -1;
        if (sl < 0) continue;
        double *o = Hc + (size_t)sl * 9;
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
    }
}

// one thread per query i of n: mask[i] bit 0 = the query's first node is fixed, bit 1 = its second; per = 9 (one 3 x 3 block per query,
// bit 0 alone) or 36 (a 6 x 6 joint block, rows / columns 0-2 the first node's, 3-5 the second's).  The rows and columns of a fixed node
// become +0 in `cov` and, where given, in `cov2` (the pinned copy the same kernel filled)
__global__ void __launch_bounds__(TPB) k_fix_cov(int n, const int *__restrict__ mask, int per, double *__restrict__ cov, double *__restrict__ cov2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = mask[i];
    if (!m || (per == 36 && isnan(cov[(size_t)36 * i]))) return;      // (a joint block marked unavailable stays marked)
    const int d = per == 9 ? 3 : 6;
    for (int r = 0; r < d; r++)
        for (int q = 0; q < d; q++)
            if ((m >> (r / 3)) & 1 || (m >> (q / 3)) & 1) {
                cov[(size_t)per * i + r * d + q] = 0.0;
                if (cov2) cov2[(size_t)per * i + r * d + q] = 0.0;
            }
}

}  // namespace asam
