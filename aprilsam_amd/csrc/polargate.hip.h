// polargate.hip.h -- part of solver.hip.cpp (included after pathsolve.hip.h).  Gating of candidate range / bearing / range-bearing
// measurements and nearest-neighbour association of the observations of one pose against landmarks.  Host driver:
// solver_gating.inc.h, launcher: launch_polar_gate (solver_launch.inc.h).
//
// Both kernels run behind the path solves (pathsolve.hip.h): `cov` holds the 6 x 6 joint blocks k_path_gram formed (k_fix_cov applied), one
// per DISTINCT pair of nodes.  The formulas are polar.h's polar_gate, shared with the host (aprilsam_amd_debug_polar_gate).  Plain loads,
// vector stores to pinned memory, no atomics, no flags; k_gate_polar uses no LDS, k_associate_polar a fixed-order LDS tree.
#pragma once
#include "polar.h"

namespace asam {

constexpr int PG_IN = 13;        // doubles per candidate of k_gate_polar: state a (3), state b (3), kind, z (2), W (4, row-major 2 x 2)
constexpr int PG_OBS = 7;        // doubles per observation of k_associate_polar: kind, z (2), W (4)
constexpr int PG_T = 256;

// One thread per candidate i of n: its block is cov[36 pidx[i]].  out: d2 at [i], S at [n + 4 i] (row-major 2 x 2; a 1-row kind writes
// [n + 4 i] and +0 behind it), 1.0 / 0.0 at [5 n + i] for a candidate that was gated / one with rho^2 == 0 (d2 and S NaN).
__global__ void __launch_bounds__(PG_T) k_gate_polar(int n, const double *__restrict__ in, const int *__restrict__ pidx, const double *__restrict__ cov,
                                                     double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *q = in + (size_t)PG_IN * i;
    double d2, S[4] = { 0.0, 0.0, 0.0, 0.0 };
    const bool ok = polar_gate((int)q[6], q + 7, q + 9, q, q + 3, cov + 36ll * pidx[i], &d2, S);
    out[i] = d2;
#pragma unroll
    for (int k = 0; k < 4; k++) out[n + 4ll * i + k] = S[k];
    out[5ll * n + i] = ok ? 1.0 : 0.0;
}

// One workgroup per observation i of m, PG_T threads; thread t gates the observation against the landmarks l = t, t + PG_T, ...: pair l's
// states are st[0..2] (the observer) and st[3 + 3 l ..], its block cov[36 l].  mat != null: d2 of (i, l) at mat[i L + l].  Each thread keeps
// its smallest d2 with its l and its second smallest, NaN skipped (ascending l and a strict <: the lower index keeps a tie); a tree over LDS
// in a fixed order merges the PG_T partial results, ties to the lower l.  Per observation:
//   res[i]   .x = the l of the smallest d2 if that is <= gate1 (one row) / gate2 (two rows), else -1;  .y = entries with rho^2 == 0
//   d2b[i], d2s[i]   the smallest and second smallest d2 over all l, +inf where there is none
__global__ void __launch_bounds__(PG_T) k_associate_polar(int L, const double *__restrict__ obs, const double *__restrict__ st, const double *__restrict__ cov,
                                                          double gate1, double gate2, double *__restrict__ mat, int2 *__restrict__ res,
                                                          double *__restrict__ d2b, double *__restrict__ d2s) {
    __shared__ double s_d1[PG_T], s_d2[PG_T];
    __shared__ int s_l[PG_T], s_nb[PG_T];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *o = obs + (size_t)PG_OBS * i;
    const int kind = (int)o[0];
    const double z[2] = { o[1], o[2] }, W[4] = { o[3], o[4], o[5], o[6] };
    const double pa[3] = { st[0], st[1], st[2] };
    double b1 = INFINITY, b2 = INFINITY;
    int l1 = -1, nb = 0;
    for (int l = tid; l < L; l += PG_T) {
        double d2, S[4];
        if (!polar_gate(kind, z, W, pa, st + 3 + 3ll * l, cov + 36ll * l, &d2, S)) nb++;
        if (mat) mat[(size_t)i * L + l] = d2;
        if (isnan(d2)) continue;
        if (d2 < b1) { b2 = b1; b1 = d2; l1 = l; }
        else if (d2 < b2) b2 = d2;
    }
    s_d1[tid] = b1; s_d2[tid] = b2; s_l[tid] = l1; s_nb[tid] = nb;
    __syncthreads();
    for (int h = PG_T / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double x1 = s_d1[tid], x2 = s_d2[tid], y1 = s_d1[tid + h], y2 = s_d2[tid + h];
            const int xl = s_l[tid], yl = s_l[tid + h];
            // (an empty side has l = -1 and d = +inf: it never wins against a finite entry, and two empty sides stay empty)
            const bool x_first = yl < 0 || (xl >= 0 && (x1 < y1 || (x1 == y1 && xl < yl)));
            if (x_first) s_d2[tid] = fmin(x2, y1);
            else { s_d1[tid] = y1; s_l[tid] = yl; s_d2[tid] = fmin(y2, x1); }
            s_nb[tid] += s_nb[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double g = polar_rows(kind) == 2 ? gate2 : gate1;
        res[i] = int2{ s_l[0] >= 0 && s_d1[0] <= g ? s_l[0] : -1, s_nb[0] };
        d2b[i] = s_d1[0]; d2s[i] = s_d2[0];
    }
}

}  // namespace asam
