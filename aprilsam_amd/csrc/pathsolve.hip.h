// pathsolve.hip.h -- joint covariances of arbitrary pose pairs from the retained factor by sparse triangular solves along
// assembly-tree paths, and the gating of candidate xyt measurements.  Host driver: solver_gating.inc.h.  DESIGN.md section 13.
//
// Sigma = A^-1 = L^-T L^-1, so for two unknowns i, j:  Sigma_ij = (L^-1 e_i)' (L^-1 e_j).  The forward solve of a unit vector e_i
// is nonzero only on the own rows of the fronts on the path from i's front to the root, so the joint block of a pair (a, b) needs
// the three columns Y_q = L^-1 e_q of each node and inner products over the paths:
//     S_aa = sum over path(a) of Y_a' Y_a,   S_bb likewise,   S_ab = sum over path(a) n path(b) (the common ancestors) of Y_a' Y_b.
// No backward solve is needed.  Every queried node gets three columns, solved once however many pairs it takes part in.
//
// Storage: per (front on a column's path, column) a dense local vector of length s + u (own rows, then real struct rows), the
// columns of one front side by side (PsFront::buf, column-major, ld = s + u).  Leaves to root, per level:
//     k_path_trsm   V_S = L_SS^-1 V_S                      one wave per (front, 16 columns); 16 x 16 tiles on v_mfma_f64_16x16x4_f64
//     k_path_gemm   parent(V_U - L_US V_S)                 one wave per (front, 16 struct rows, 16 columns); written through front_rel
//                                                          into the parent's local vectors (each element by exactly one lane)
// then k_path_gram forms the 6 x 6 blocks and k_gate_xyt the innovation covariance and Mahalanobis distance of each candidate.
// Every sum runs in a fixed order, without atomics: two calls give the same bits.  The factor is only read.
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

struct PsFront {
    long long off;             // frontal array in the factor pool (leading dimension R)
    long long buf;             // the local vectors in the work buffer: (s + u) x ncol, column-major
    int s, u, R, ncol;         // own rows, real struct rows (scalars), pool leading dimension, columns through this front
    int parent;                // record of the parent front (-1: root)
    int rel_begin;             // the struct rows' blocks inside the parent's row list (front_rel) at this offset of the int arena
    int cmap;                  // per column: its index among the parent's columns, at this offset of the column map
    int first;                 // first own position (the tree solve's tables: treesolve.hip.h)
};
static_assert(sizeof(PsFront) == 48, "PsFront layout");

struct PsPath { long long col0; int ld, s; };         // one front on a node's path: its first column's own rows
struct PsPair { int pa, na, pb, nb, nc, out; };       // path entries of a and b, the common ancestors (the last nc of both), output slot

// One wave per ent = { record, column tile }: V_S = L_SS^-1 V_S on 16 columns (tile_trsm, selinv.hip.h).
__global__ void __launch_bounds__(256) k_path_trsm(const PsFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                   double *__restrict__ buf) {
    __shared__ double T[4][SEL_T][SEL_T + 1];
    const int w = sel_wave(n);
    if (w < 0) return;
    const int4 e = ent[w];
    const PsFront F = fr[e.x];
    const int ld = F.s + F.u, c0 = SEL_T * e.y;
    tile_trsm<false>(pool + F.off, F.R, F.s, buf + F.buf + (long long)c0 * ld, ld, min(SEL_T, F.ncol - c0), T[threadIdx.x >> 6]);
}

// One wave per ent = { record, struct-row tile, column tile }: W = V_U - L_US V_S, element (a, c) stored at the parent's local row
// 3 rel[a / 3] + a % 3 of the parent's column cmap[c] (the extend-add's map).  A column passes through one child of each front on
// its path, so every element of a parent's local vectors is written at most once; the rest stay zero.
__global__ void __launch_bounds__(256) k_path_gemm(const PsFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                   const int *__restrict__ rel, const int *__restrict__ cmap, double *__restrict__ buf) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const int4 e = ent[w];
    const PsFront F = fr[e.x], P = fr[F.parent];
    const int s = F.s, u = F.u, R = F.R, ld = s + u, ldp = P.s + P.u, i0 = SEL_T * e.y, c0 = SEL_T * e.z;
    const double *Lus = pool + F.off + s;
    const double *V = buf + F.buf;
    sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
    acc = sel_mma([&](int i, int k) { return i0 + i < u ? Lus[(long long)k * R + i0 + i] : 0.0; },
                  [&](int k, int c) { return c0 + c < F.ncol ? V[(long long)(c0 + c) * ld + k] : 0.0; }, 0, s, acc);
    const int *rl = rel + F.rel_begin;
    sel_tile_store(i0, c0, u, F.ncol, acc, [&](int row, int col, double v) {
        const int pr = 3 * rl[row / 3] + row % 3, pc = cmap[F.cmap + col];
        if (pr < ldp && pc >= 0 && pc < P.ncol)                // (the host tables promise both; a broken map must not write elsewhere)
            buf[P.buf + (long long)pc * ldp + pr] = V[(long long)col * ld + s + row] - v;
    });
}

// the right-hand sides: a one at each listed element of the zeroed work buffer (three per node, in its own front)
__global__ void __launch_bounds__(256) k_path_init(int n, const long long *__restrict__ at, double *__restrict__ buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) buf[at[i]] = 1.0;
}

// One workgroup per pair: the 21 distinct inner products of [Y_a Y_b], each thread over rows tid, tid + 256, ... of the path
// entries in order, then a fixed tree in LDS.  Writes the 6 x 6 block (row-major, a's unknowns first) to cov (device, for the gate)
// and to out (pinned host memory).
__global__ void __launch_bounds__(256) k_path_gram(const PsPair *__restrict__ pairs, const PsPath *__restrict__ path, const double *__restrict__ buf,
                                                   double *__restrict__ cov, double *__restrict__ out) {
    __shared__ double red[21][256];
    const PsPair p = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    double acc[21];
#pragma unroll
    for (int q = 0; q < 21; q++) acc[q] = 0.0;
    // acc[0..6) = aa (00 01 02 11 12 22), acc[6..12) = bb, acc[12..21) = ab (row-major)
    auto sym = [&](double *a6, const double *y) {
        a6[0] += y[0] * y[0]; a6[1] += y[0] * y[1]; a6[2] += y[0] * y[2]; a6[3] += y[1] * y[1]; a6[4] += y[1] * y[2]; a6[5] += y[2] * y[2];
    };
    for (int q = 0; q < p.na - p.nc; q++) {
        const PsPath E = path[p.pa + q];
        for (int r = tid; r < E.s; r += 256) {
            const double y[3] = { buf[E.col0 + r], buf[E.col0 + E.ld + r], buf[E.col0 + 2ll * E.ld + r] };
            sym(acc, y);
        }
    }
    for (int q = 0; q < p.nb - p.nc; q++) {
        const PsPath E = path[p.pb + q];
        for (int r = tid; r < E.s; r += 256) {
            const double y[3] = { buf[E.col0 + r], buf[E.col0 + E.ld + r], buf[E.col0 + 2ll * E.ld + r] };
            sym(acc + 6, y);
        }
    }
    for (int q = 0; q < p.nc; q++) {
        const PsPath Ea = path[p.pa + p.na - p.nc + q], Eb = path[p.pb + p.nb - p.nc + q];
        for (int r = tid; r < Ea.s; r += 256) {
            const double ya[3] = { buf[Ea.col0 + r], buf[Ea.col0 + Ea.ld + r], buf[Ea.col0 + 2ll * Ea.ld + r] };
            const double yb[3] = { buf[Eb.col0 + r], buf[Eb.col0 + Eb.ld + r], buf[Eb.col0 + 2ll * Eb.ld + r] };
            sym(acc, ya); sym(acc + 6, yb);
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) acc[12 + 3 * i + j] += ya[i] * yb[j];
        }
    }
#pragma unroll
    for (int q = 0; q < 21; q++) red[q][tid] = acc[q];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st)
#pragma unroll
            for (int q = 0; q < 21; q++) red[q][tid] += red[q][tid + st];
        __syncthreads();
    }
    if (tid < 36) {
        const int r = tid / 6, c = tid % 6;
        const int ri = r % 3, ci = c % 3, lo = min(ri, ci), hi = max(ri, ci);
        const int sidx = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);          // (00 01 02 11 12 22)
        double v;
        if (r < 3 && c < 3) v = red[sidx][0];
        else if (r >= 3 && c >= 3) v = red[6 + sidx][0];
        else if (r < 3) v = red[12 + 3 * ri + ci][0];                   // S_ab
        else v = red[12 + 3 * ci + ri][0];                              // S_ba = S_ab'
        cov[36ll * p.out + tid] = v;
        out[36ll * p.out + tid] = v;
    }
}

// out (3 x 3, row-major) = [J0 J1] C [J0 J1]': the covariance of an xyt prediction with the Jacobians J0, J1 (3 x 3 each) under the joint
// block C (6 x 6) of its two poses.  Jc = [J0 J1], then Jc C, then the product with Jc', every sum over k ascending.
__device__ __forceinline__ void xyt_joint_cov(const double *J0, const double *J1, const double *C, double *out) {
    double Jc[18], JC[18];                                // 3 x 6 row-major
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) { Jc[6 * a + b] = J0[3 * a + b]; Jc[6 * a + 3 + b] = J1[3 * a + b]; }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v += Jc[6 * a + k] * C[6 * k + b];
            JC[6 * a + b] = v;
        }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v += JC[6 * a + k] * Jc[6 * b + k];
            out[3 * a + b] = v;
        }
}

// wi = W^-1 (3 x 3, row-major) by the adjugate, nine quotients by det W, which is returned: what every gate of xyt candidates adds to
// its innovation covariance, and the gain takes the logarithm of
__device__ __forceinline__ double xyt_info_inverse(const double *W, double *wi) {
    const double det = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
    wi[0] = (W[4] * W[8] - W[5] * W[7]) / det; wi[1] = (W[2] * W[7] - W[1] * W[8]) / det; wi[2] = (W[1] * W[5] - W[2] * W[4]) / det;
    wi[3] = (W[5] * W[6] - W[3] * W[8]) / det; wi[4] = (W[0] * W[8] - W[2] * W[6]) / det; wi[5] = (W[2] * W[3] - W[0] * W[5]) / det;
    wi[6] = (W[3] * W[7] - W[4] * W[6]) / det; wi[7] = (W[1] * W[6] - W[0] * W[7]) / det; wi[8] = (W[0] * W[4] - W[1] * W[3]) / det;
    return det;
}

// One thread per candidate (a, b, z, W): in = { state a (3), state b (3), z (3), W (9, row-major) }, cov its joint block.
//   r, J_a, J_b    the xyt factor's residual (theta wrapped) and Jacobians at the states (factor_residual)
//   S = [J_a J_b] cov [J_a J_b]' + W^-1,   d2 = r' S^-1 r   (Cholesky of S)
// out: d2 at [i], S (row-major) at [n + 9 i].
__global__ void __launch_bounds__(256) k_gate_xyt(int n, const double *__restrict__ in, const double *__restrict__ cov, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *q = in + 18ll * i, *C = cov + 36ll * i;
    double J0[9], J1[9], r[3];
    factor_residual(true, q, q + 3, q + 6, J0, J1, r);
    double Wi[9];
    xyt_info_inverse(q + 9, Wi);                          // (W was checked positive definite on the host)
    double S[9];
    xyt_joint_cov(J0, J1, C, S);
#pragma unroll
    for (int k = 0; k < 9; k++) S[k] = S[k] + Wi[k];
    const double l00 = sqrt(S[0]), l10 = S[3] / l00, l20 = S[6] / l00;
    const double l11 = sqrt(S[4] - l10 * l10), l21 = (S[7] - l20 * l10) / l11;
    const double l22 = sqrt(S[8] - l20 * l20 - l21 * l21);
    const double y0 = r[0] / l00, y1 = (r[1] - l10 * y0) / l11, y2 = (r[2] - l20 * y0 - l21 * y1) / l22;
    out[i] = y0 * y0 + y1 * y1 + y2 * y2;
#pragma unroll
    for (int k = 0; k < 9; k++) out[n + 9ll * i + k] = S[k];
}

}  // namespace asam
