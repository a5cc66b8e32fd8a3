// gaussian.hip.h -- part of solver.hip.cpp (included after polar.hip.h).  Dense Gaussian factors on k nodes, information form (DESIGN.md
// section 24).
//
// A packed Gaussian factor occupies the entries of the clique of its node pairs -- k (k - 1) / 2 of them in the order (0,1), (0,2), ...,
// (1,2), ...; one unary entry for k = 1 -- whose slots of d_z / d_W hold a null factor, so k_linearize_t writes zero contributions there.
// Its data lives in a table of its own (GraphPack::gs_*, fixed-width rows padded to GS_MAX nodes):
//   gf[q]            first packed entry of Gaussian factor q
//   gk[q]            k
//   gnode[11 q]      the node ids
//   gxbar[33 q]      xbar,  geta[33 q]  eta
//   gL[1089 q]       Lambda, 3k x 3k row-major with row stride 3k
//   gc0[q]           the chi^2 constant
// k_gaussian_slot writes Lambda's blocks and g = eta - Lambda delta (delta at the l_points) into the entries' contribution slots after
// k_linearize_t and before k_fix_mask, in k_scatter_host's layout: entry (x, y) carries the off-diagonal block (x, y); node 0's and node 1's
// diagonal block and rhs segment ride on (0, 1), node y's on (0, y); what an entry does not carry is written as zeros.  k_chi2_gaussian
// puts the factor's term at the states on its first entry and 0 on the others; k_lm_model_gaussian does the same for LM's model decrease.
// One wave per factor; each lane sums its row in ascending column order and lane 0 sums the rows in ascending order: no atomics, two runs
// give the same bits.
#pragma once

namespace asam {

constexpr int GS_MAX = 11;                      // nodes per factor (APRILSAM_AMD_GAUSSIAN_MAX_NODES: the clique limit of pack_factors)
constexpr int GS_ROWS = 3 * GS_MAX;             // 33
constexpr int GS_LSZ = GS_ROWS * GS_ROWS;       // 1089

// the table as the kernels take it
struct GaussTab { int G; const int *gf, *gk, *gnode; const double *gxbar, *geta, *gL, *gc0; };

// delta = pts (-) xbar of factor q into sd[0, 3k), by the lanes r < 3k; the wave's LDS writes are complete on return
__device__ __forceinline__ void gaussian_delta(const GaussTab &t, int q, int k, const double *__restrict__ pts, double *sd) {
    const int r = threadIdx.x;
    if (r < 3 * k) {
        const int node = t.gnode[GS_MAX * q + r / 3], c = r - 3 * (r / 3);
        const double v = pts[(size_t)3 * node + c] - t.gxbar[(size_t)GS_ROWS * q + r];
        sd[r] = c == 2 ? mod2pi_dev(v) : v;
    }
    __syncthreads();
}
// (Lambda v)_r for the lane's row r < 3k, ascending columns
__device__ __forceinline__ double gaussian_row(const GaussTab &t, int q, int k, int r, const double *v) {
    const int n = 3 * k;
    const double *L = t.gL + (size_t)GS_LSZ * q + (size_t)r * n;
    double acc = 0;
    for (int j = 0; j < n; j++) acc += L[j] * v[j];
    return acc;
}

__global__ void __launch_bounds__(64) k_gaussian_slot(GaussTab t, const double *__restrict__ lp, const unsigned char *__restrict__ swp,
                                                      const int *__restrict__ slot_blk, const int *__restrict__ slot_rhs, double *__restrict__ Hc) {
    __shared__ double sd[GS_ROWS], sg[GS_ROWS];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= t.G) return;
    const int k = t.gk[q], n = 3 * k, f0 = t.gf[q];
    gaussian_delta(t, q, k, lp, sd);
    if (lane < n) sg[lane] = t.geta[(size_t)GS_ROWS * q + lane] - gaussian_row(t, q, k, lane, sd);
    __syncthreads();
    const int ne = k == 1 ? 1 : k * (k - 1) / 2;
    if (lane >= ne) return;
    int x = 0, y = 1;
    if (k > 1) { int rem = lane; while (rem >= k - 1 - x) { rem -= k - 1 - x; x++; } y = x + 1 + rem; }
    const int f = f0 + lane;
    const bool ca = k == 1 || (x == 0 && y == 1), cb = k > 1 && x == 0;      // what the entry carries: x's / y's diagonal block and rhs
    const double *L = t.gL + (size_t)GS_LSZ * q;
    double *o = Hc + (size_t)slot_blk[3 * f] * 9, *go = Hc + (size_t)slot_rhs[2 * f] * 9;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o[i * 3 + j] = ca ? L[(size_t)(3 * x + i) * n + 3 * x + j] : 0.0;
        go[i] = ca ? sg[3 * x + i] : 0.0;
    }
    if (k == 1) return;
    const bool s = swp[f] & 1;
    double *o1 = Hc + (size_t)slot_blk[3 * f + 1] * 9, *o2 = Hc + (size_t)slot_blk[3 * f + 2] * 9, *g1 = Hc + (size_t)slot_rhs[2 * f + 1] * 9;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            o1[i * 3 + j] = s ? L[(size_t)(3 * x + j) * n + 3 * y + i] : L[(size_t)(3 * x + i) * n + 3 * y + j];      // rows x, columns y; transposed when y is eliminated later
            o2[i * 3 + j] = cb ? L[(size_t)(3 * y + i) * n + 3 * y + j] : 0.0;
        }
        g1[i] = cb ? sg[3 * y + i] : 0.0;
    }
}

// c0 - 2 eta' delta + delta' Lambda delta at st -> out[first entry], 0 -> out[the other entries].  The rounding of a term that is zero in
// exact arithmetic is cut off at 0 (LM's objective stays non-negative)
__global__ void __launch_bounds__(64) k_chi2_gaussian(GaussTab t, const double *__restrict__ st, double *__restrict__ out) {
    __shared__ double sd[GS_ROWS], sv[GS_ROWS];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= t.G) return;
    const int k = t.gk[q], n = 3 * k, f0 = t.gf[q];
    gaussian_delta(t, q, k, st, sd);
    if (lane < n) sv[lane] = sd[lane] * (gaussian_row(t, q, k, lane, sd) - 2.0 * t.geta[(size_t)GS_ROWS * q + lane]);
    __syncthreads();
    const int ne = k == 1 ? 1 : k * (k - 1) / 2;
    if (lane == 0) {
        double acc = t.gc0[q];
        for (int r = 0; r < n; r++) acc += sv[r];
        out[f0] = acc > 0 ? acc : 0.0;
    } else if (lane < ne) out[f0 + lane] = 0.0;
}

// LM's model decrease of the factor: h' (2 g - Lambda h) with g = eta - Lambda delta at lp and h = dx of its nodes -> out[first entry]
// (the other entries hold the 0 that k_lm_model made of their null slots, and are written again as such)
__global__ void __launch_bounds__(64) k_lm_model_gaussian(GaussTab t, const double *__restrict__ lp, const double *__restrict__ dx, double *__restrict__ out) {
    __shared__ double sd[GS_ROWS], sh[GS_ROWS], sv[GS_ROWS];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= t.G) return;
    const int k = t.gk[q], n = 3 * k, f0 = t.gf[q];
    if (lane < n) sh[lane] = dx[(size_t)3 * t.gnode[GS_MAX * q + lane / 3] + lane % 3];
    gaussian_delta(t, q, k, lp, sd);
    if (lane < n) {
        const double g = t.geta[(size_t)GS_ROWS * q + lane] - gaussian_row(t, q, k, lane, sd);
        sv[lane] = sh[lane] * (2.0 * g - gaussian_row(t, q, k, lane, sh));
    }
    __syncthreads();
    const int ne = k == 1 ? 1 : k * (k - 1) / 2;
    if (lane == 0) {
        double acc = 0;
        for (int r = 0; r < n; r++) acc += sv[r];
        out[f0] = acc;
    } else if (lane < ne) out[f0 + lane] = 0.0;
}

// ---- the marginal prior of a node set from the retained linearisation (aprilsam_amd_marginal_prior; solver_marginal_prior.inc.h) ----
// One workgroup.  The n = nm + nb nodes of M (local rows [0, nm)) and of its blanket B (rows [nm, n)) span the dense system T = [H | g],
// 3n x (3n + 1) doubles in LDS (MP_MAX_NODES = 40: 116 KB).  ent[3e] = (packed entry, local row of a, local row of b or -1) lists the
// entries that touch M, ascending: their slots of Hc are added one entry after the other (33 lanes, each on a location of its own, a barrier
// between entries: the sums have one order).  The diagonal slots hold the symmetrised full block, the off-diagonal slot is in final
// orientation (swp).  No lambda, no damping: the slots alone.
// Elimination, right-looking on the augmented system: for column j of the M block, u = row j / sqrt(T_jj) (fast_rsqrt, as the factorisation's
// chains) -- the Cholesky row and, in the columns of B and g, the triangular solve -- then T_ic -= u_i u_c for i, c > j: after 3 nm steps the
// B block holds Lambda = H_BB - H_BM H_MM^-1 H_MB and the last column eta = g_B - H_BM H_MM^-1 g_M.  A pivot that is not positive or not
// finite: bad[0] = 1, bad[1] = j, nothing written.  Output: xbar (lp of B's nodes, 3 nb), eta (3 nb), Lambda (3 nb x 3 nb, from the upper triangle).
constexpr int MP_MAX_NODES = 40;
constexpr int MP_THREADS = 256;
__global__ void __launch_bounds__(MP_THREADS) k_marginal_prior(int nE, const int *__restrict__ ent, int nm, int nb, const int *__restrict__ keep,
                                                               const unsigned char *__restrict__ swp, const int *__restrict__ slot_blk,
                                                               const int *__restrict__ slot_rhs, const double *__restrict__ Hc, const double *__restrict__ lp,
                                                               double *__restrict__ out, int *__restrict__ bad) {
    extern __shared__ double mp_lds[];
    const int n3 = 3 * (nm + nb), m3 = 3 * nm, b3 = 3 * nb, ld = n3 + 1, tid = threadIdx.x;
    double *T = mp_lds, *U = mp_lds + (size_t)n3 * ld;
    for (int i = tid; i < n3 * ld; i += MP_THREADS) T[i] = 0.0;
    __syncthreads();
    for (int e = 0; e < nE; e++) {
        const int f = ent[3 * e], ra = 3 * ent[3 * e + 1], rb = 3 * ent[3 * e + 2];
        if (tid < 33 && (rb >= 0 || tid < 9 || (tid >= 27 && tid < 30))) {
            if (tid < 9) { const int i = tid / 3, j = tid % 3; T[(ra + i) * ld + ra + j] += Hc[(size_t)slot_blk[3 * f] * 9 + tid]; }
            else if (tid < 18) {
                const int i = (tid - 9) / 3, j = (tid - 9) % 3;         // H_ab[i][j]: rows a, columns b
                const double v = Hc[(size_t)slot_blk[3 * f + 1] * 9 + ((swp[f] & 1) ? j * 3 + i : i * 3 + j)];
                T[(ra + i) * ld + rb + j] += v; T[(rb + j) * ld + ra + i] += v;
            }
            else if (tid < 27) { const int i = (tid - 18) / 3, j = (tid - 18) % 3; T[(rb + i) * ld + rb + j] += Hc[(size_t)slot_blk[3 * f + 2] * 9 + tid - 18]; }
            else if (tid < 30) T[(ra + tid - 27) * ld + n3] += Hc[(size_t)slot_rhs[2 * f] * 9 + tid - 27];
            else T[(rb + tid - 30) * ld + n3] += Hc[(size_t)slot_rhs[2 * f + 1] * 9 + tid - 30];
        }
        __syncthreads();
    }
    for (int j = 0; j < m3; j++) {
        const double d = T[j * ld + j];
        if (!(d > 0) || !(d < 1.0e308)) {            // (uniform: every thread reads the same pivot)
            if (tid == 0) { bad[0] = 1; bad[1] = j; }
            return;
        }
        const double r = fast_rsqrt(d);
        for (int c = j + 1 + tid; c <= n3; c += MP_THREADS) U[c] = T[j * ld + c] * r;
        __syncthreads();
        const int w = n3 - j;                        // columns j + 1 .. n3 of the rows j + 1 .. n3 - 1
        for (int t = tid; t < (w - 1) * w; t += MP_THREADS) {
            const int i = j + 1 + t / w, c = j + 1 + t % w;
            T[i * ld + c] -= U[i] * U[c];
        }
        __syncthreads();
    }
    for (int t = tid; t < b3; t += MP_THREADS) {
        out[t] = lp[(size_t)3 * keep[t / 3] + t % 3];
        out[b3 + t] = T[(m3 + t) * ld + n3];
    }
    for (int t = tid; t < b3 * b3; t += MP_THREADS) {
        const int i = t / b3, c = t % b3;
        out[2 * b3 + t] = T[(m3 + (i < c ? i : c)) * ld + m3 + (i < c ? c : i)];
    }
}

}  // namespace asam
