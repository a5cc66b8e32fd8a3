// treesolve.hip.h -- solves with the retained factor for right-hand sides the caller supplies (A X = B and the half-solves L^-1, L^-T
// in node coordinates), and what is read from such a solve: the cross-covariances of every pose with an anchor pose and the covariances
// of every pose relative to it.  Host driver: solver_treesolve.inc.h.  DESIGN.md section 18.
//
// A = P' L L' P (P: node order -> elimination order).  Every column of B passes through EVERY front of the assembly tree, so each front
// gets a dense local block of (s + u) x ncol (own rows, then the real struct rows; column-major, ld = s + u) in one work buffer: what
// PsFront::buf is for the path solves (pathsolve.hip.h), without a column map.  Here PsFront::buf holds the front's first ROW in the
// buffer and the kernels take the column count as an argument (block = buf * ncol): the table does not depend on the chunk width; buf / 3
// is the front's first block row in the global list of block rows (the children CSR), PsFront::first its first own position.  One launch
// per kernel and level; fronts are grouped by their depth below the root and a kernel boundary orders the levels.
//   forward, leaves to root     k_ts_assemble   own rows = B (node -> pos -> local row); all rows += the children's finished V_U, child
//                                               by child in ascending front id (a parent-side gather through front_rel: several children
//                                               contribute to the same parent row)
//                               k_ts_trsm       V_S = L_SS^-1 V_S            (tile_trsm<false>, as k_path_trsm; column tile from the grid)
//                               k_ts_gemm       V_U = V_U - L_US V_S         (into the front's OWN block)
//   backward, root to leaves    k_ts_gather     V_U = the parent's solved values at the front_rel rows (single reader)
//                               k_ts_gemmt      V_S = V_S - L_US' V_U
//                               k_ts_trsmt      V_S = L_SS^-T V_S            (tile_trsm<true>: row blocks from the last to the first)
//   k_ts_store / k_cross_extract / k_relative_cov read the own rows.
// Every output element is written by exactly one lane from a sum in a fixed order (the MFMA k loop, the children in ascending id): no
// atomics, no flags; two calls give the same bits, and a column's arithmetic does not depend on its neighbours in a tile, so the
// results do not depend on how the columns are chunked.  The factor is only read; partial tiles are predicated.
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

constexpr int TS_BAND = 64;                // rows per work entry of the element-wise kernels (one wave's lanes)

struct TsKid { int wrow, ld, off, pad; };  // one contribution to a parent block row: the child's first row in the buffer (x ncol), its ld, s + 3 a

// ent = { front, band of 64 local rows }; a wave's lanes are consecutive rows, its four waves stride the columns.
// own rows: B[col][3 node + k] (load != 0), else 0; then every row adds the children's V_U in ascending front id (kids != 0).
__global__ void __launch_bounds__(256) k_ts_assemble(const PsFront *__restrict__ fr, const int2 *__restrict__ ent,
                                                     const int *__restrict__ cptr, const TsKid *__restrict__ cent, const int *__restrict__ node_of_pos,
                                                     const double *__restrict__ B, long long n3, int load, int kids, int ncol, double *__restrict__ buf) {
    const int2 e = ent[blockIdx.x];
    const PsFront F = fr[e.x];
    const int ld = F.s + F.u, row = TS_BAND * e.y + (threadIdx.x & 63);
    if (row >= ld) return;
    const int blk = row / 3, k = row % 3, brow0 = (int)F.buf / 3;      // (the buffer's rows fit an int: ts_tables)
    const int q0 = kids ? cptr[brow0 + blk] : 0, q1 = kids ? cptr[brow0 + blk + 1] : 0;
    const long long brow = (load && row < F.s) ? 3ll * node_of_pos[F.first + blk] + k : -1;
    for (int col = threadIdx.x >> 6; col < ncol; col += 4) {
        double v = brow >= 0 ? B[(long long)col * n3 + brow] : 0.0;
        for (int q = q0; q < q1; q++) {
            const TsKid c = cent[q];
            v += buf[(long long)c.wrow * ncol + (long long)col * c.ld + c.off + k];
        }
        buf[F.buf * ncol + (long long)col * ld + row] = v;
    }
}

// One wave per (ent = { front, - }, 16 columns: column tile blockIdx.y): V_S = L_SS^-1 V_S, TRANS: L_SS^-T V_S (tile_trsm, selinv.hip.h).
template <bool TRANS>
__device__ __forceinline__ void ts_trsm(const PsFront *__restrict__ fr, const int2 *__restrict__ ent, int n, const double *__restrict__ pool, int ncol,
                                        double *__restrict__ buf) {
    __shared__ double T[4][SEL_T][SEL_T + 1];
    const int w = sel_wave(n);
    if (w < 0) return;
    const PsFront F = fr[ent[w].x];
    const int ld = F.s + F.u, c0 = SEL_T * blockIdx.y;
    tile_trsm<TRANS>(pool + F.off, F.R, F.s, buf + F.buf * ncol + (long long)c0 * ld, ld, min(SEL_T, ncol - c0), T[threadIdx.x >> 6]);
}
__global__ void __launch_bounds__(256) k_ts_trsm(const PsFront *__restrict__ fr, const int2 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                 int ncol, double *__restrict__ buf) {
    ts_trsm<false>(fr, ent, n, pool, ncol, buf);
}
__global__ void __launch_bounds__(256) k_ts_trsmt(const PsFront *__restrict__ fr, const int2 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                  int ncol, double *__restrict__ buf) {
    ts_trsm<true>(fr, ent, n, pool, ncol, buf);
}

// One wave per (ent = { front, struct-row tile }, column tile blockIdx.y): V_U = V_U - L_US V_S, k_path_gemm's product written into
// the front's own block.
__global__ void __launch_bounds__(256) k_ts_gemm(const PsFront *__restrict__ fr, const int2 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                 int ncol, double *__restrict__ buf) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const int2 e = ent[w];
    const PsFront F = fr[e.x];
    const int s = F.s, u = F.u, R = F.R, ld = s + u, i0 = SEL_T * e.y, c0 = SEL_T * blockIdx.y;
    if (c0 >= ncol) return;
    const double *Lus = pool + F.off + s;
    double *V = buf + F.buf * ncol;
    sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
    acc = sel_mma([&](int i, int k) { return i0 + i < u ? Lus[(long long)k * R + i0 + i] : 0.0; },
                  [&](int k, int c) { return c0 + c < ncol ? V[(long long)(c0 + c) * ld + k] : 0.0; }, 0, s, acc);
    sel_tile_store(i0, c0, u, ncol, acc, [&](int row, int col, double v) { V[(long long)col * ld + s + row] = V[(long long)col * ld + s + row] - v; });
}

// ent = { front, band of 64 struct rows }: V_U[a] = the parent's local row 3 rel[a / 3] + a % 3 (k_selinv_gather's map), every column.
__global__ void __launch_bounds__(256) k_ts_gather(const PsFront *__restrict__ fr, const int *__restrict__ rel, const int2 *__restrict__ ent,
                                                   int ncol, double *__restrict__ buf) {
    const int2 e = ent[blockIdx.x];
    const PsFront F = fr[e.x], P = fr[F.parent];
    const int ld = F.s + F.u, ldp = P.s + P.u, a = TS_BAND * e.y + (threadIdx.x & 63);
    if (a >= F.u) return;
    const int pr = 3 * rel[F.rel_begin + a / 3] + a % 3;
    if (pr < 0 || pr >= ldp) return;                      // (the host tables promise it; a broken map must not read elsewhere)
    for (int col = threadIdx.x >> 6; col < ncol; col += 4)
        buf[F.buf * ncol + (long long)col * ld + F.s + a] = buf[P.buf * ncol + (long long)col * ldp + pr];
}

// One wave per (ent = { front, own-row tile }, column tile blockIdx.y): V_S = V_S - L_US' V_U, K over the u struct rows.
__global__ void __launch_bounds__(256) k_ts_gemmt(const PsFront *__restrict__ fr, const int2 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                  int ncol, double *__restrict__ buf) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const int2 e = ent[w];
    const PsFront F = fr[e.x];
    const int s = F.s, u = F.u, R = F.R, ld = s + u, i0 = SEL_T * e.y, c0 = SEL_T * blockIdx.y;
    if (c0 >= ncol) return;
    const double *Lus = pool + F.off + s;                 // L_US[k][i] = Lus[k + i R]
    double *V = buf + F.buf * ncol;
    sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
    acc = sel_mma([&](int i, int k) { return i0 + i < s ? Lus[(long long)(i0 + i) * R + k] : 0.0; },
                  [&](int k, int c) { return c0 + c < ncol ? V[(long long)(c0 + c) * ld + s + k] : 0.0; }, 0, u, acc);
    sel_tile_store(i0, c0, s, ncol, acc, [&](int row, int col, double v) { V[(long long)col * ld + row] = V[(long long)col * ld + row] - v; });
}

// the own-row element of node `node`'s unknown k in column col
__device__ __forceinline__ double ts_value(const PsFront *__restrict__ fr, const int *__restrict__ pos,
                                           const int *__restrict__ pos_front, const double *__restrict__ buf, int ncol, int node, int k, int col) {
    const int p = pos[node], t = pos_front[p];
    const PsFront F = fr[t];
    return buf[F.buf * ncol + (long long)col * (F.s + F.u) + 3 * (p - F.first) + k];
}

// X[col][3 node + k] in node order, one thread per value, straight into pinned host memory.
__global__ void __launch_bounds__(256) k_ts_store(const PsFront *__restrict__ fr, const int *__restrict__ pos,
                                                  const int *__restrict__ pos_front, const double *__restrict__ buf, int N, int ncol,
                                                  double *__restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x, n3 = 3ll * N;
    if (g >= n3 * ncol) return;
    const int i = (int)(g % n3), col = (int)(g / n3);
    out[g] = ts_value(fr, pos, pos_front, buf, ncol, i / 3, i % 3, col);
}

// Sigma_{node, anchor} (row-major, the node's unknowns as rows) from the FULL solve of the anchor's three unit columns: one thread per
// value.  nodes == null: node p is p.
__global__ void __launch_bounds__(256) k_cross_extract(int n, const int *__restrict__ nodes, const PsFront *__restrict__ fr,
                                                       const int *__restrict__ pos, const int *__restrict__ pos_front, const double *__restrict__ buf,
                                                       double *__restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 9ll * n) return;
    const int p = (int)(g / 9), e = (int)(g % 9);
    out[g] = ts_value(fr, pos, pos_front, buf, 3, nodes ? nodes[p] : p, e / 3, e % 3);
}

// One thread per listed node i: the covariance of the predicted xyt measurement x_anchor^-1 o x_i,
//     [J_a J_i] [[Sig_aa Sig_ai]; [Sig_ia Sig_ii]] [J_a J_i]'
// with the Jacobians an xyt factor computes at the states st_a / st[3 p..] (factor_residual, as k_gate_xyt takes them: the result is
// k_gate_xyt's S - W^-1), Sig_aa and Sig_ii from the Sigma pool (k_marginal_extract's read) and Sig_ia from the solve.  i == anchor: zeros.
__global__ void __launch_bounds__(256) k_relative_cov(int n, const int *__restrict__ nodes, int anchor, const double *__restrict__ st_a,
                                                      const double *__restrict__ st, const PsFront *__restrict__ fr,
                                                      const int *__restrict__ pos, const int *__restrict__ pos_front, const double *__restrict__ buf,
                                                      const double *__restrict__ sig, double *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int node = nodes ? nodes[p] : p;
    double *o = out + 9ll * p;
    if (node == anchor) {
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = 0.0;
        return;
    }
    double C[36];                                         // the joint block, the anchor's unknowns first
    auto diag = [&](int q, int at) {
        const int pq = pos[q], t = pos_front[pq];
        const PsFront F = fr[t];
        const int l = 3 * (pq - F.first);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) C[6 * (at + r) + at + c] = sig[F.off + (long long)(l + c) * F.R + l + r];
    };
    diag(anchor, 0); diag(node, 3);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v = ts_value(fr, pos, pos_front, buf, 3, node, r, c);      // Sig_ia[r][c]
            C[6 * (3 + r) + c] = v; C[6 * c + 3 + r] = v;
        }
    const double z[3] = { 0.0, 0.0, 0.0 };
    double J0[9], J1[9], res[3];
    factor_residual(true, st_a, st + 3ll * p, z, J0, J1, res);
    xyt_joint_cov(J0, J1, C, o);
}

}  // namespace asam
