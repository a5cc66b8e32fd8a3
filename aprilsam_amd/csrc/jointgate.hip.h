// jointgate.hip.h -- part of solver.hip.cpp (included after pathsolve.hip.h).  Joint compatibility gating of closure hypotheses
// (aprilsam_amd_gate_xyt_joint): the Mahalanobis distance of the stacked residual of a SET of candidate xyt measurements under their full
// joint innovation covariance, cross terms included.  Host driver: solver_gating.inc.h.  DESIGN.md section 29.
//
// k_gate_xyt_joint runs behind the path solves (pathsolve.hip.h): `cov` holds the 6 x 6 joint blocks k_path_gram formed (k_fix_cov applied),
// one per DISTINCT unordered node pair of the call.  One workgroup of one wave per hypothesis of m <= JG_MAX candidates, n = 3 m rows:
//     r_i, J_ai, J_bi, W_i^-1        per candidate, exactly as k_gate_xyt takes them (factor_residual, the adjugate)
//     C(i, j) = [J_ai J_bi] [[S(a_i,a_j) S(a_i,b_j)]; [S(b_i,a_j) S(b_i,b_j)]] [J_aj J_bj]'  (+ W_i^-1 on the diagonal)
//                                    one thread per lower 3 x 3 block; the four S come through the index table: entry = 4 slot + sub,
//                                    sub picking the 3 x 3 quarter of the slot's block (1: rows 0..2 / columns 3..5, 2: the mirror quarter
//                                    -- the same pair read the other way round --, 0 / 3: the diagonal quarters)
//     C = L L', y = L^-1 r           by columns, thread t owning row t; prefix j = sum of y_t^2 over t < 3 (j + 1)
// C, r and the Jacobians stay in LDS.  C's leading dimension JG_LD is odd: thread t walks row t (ds_read_b64 at a stride of 2 JG_LD dwords,
// 32 lanes on 32 distinct bank pairs), the pivot row is one address for all lanes (a broadcast).  Every sum runs over k ascending in one
// thread, no atomics, no reduction whose shape depends on m: element (t, c) of L and y_c take the same operations whatever follows them, so
// a hypothesis cut to its first j candidates reproduces prefix j bit for bit, and two calls give the same bits.  Plain vector stores to
// pinned memory.  The host promises 1 <= m <= JG_MAX and table entries inside cov; a broken table is not run (the guards below return).
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

constexpr int JG_MAX = 16;       // candidates per hypothesis (APRILSAM_AMD_JOINT_MAX)
constexpr int JG_N = 3 * JG_MAX; // rows of the largest C
constexpr int JG_LD = JG_N + 1;  // odd: see above
constexpr int JG_T = 64;         // one wave

// out (3 x 3, row-major) = [Ji0 Ji1] C [Jj0 Jj1]' for a 6 x 6 C: xyt_joint_cov's sums (k ascending) with another right-hand pair
__device__ __forceinline__ void xyt_cross_cov(const double *Ji0, const double *Ji1, const double *C, const double *Jj0, const double *Jj1, double *out) {
    double JC[18];                                        // 3 x 6 row-major
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v += (k < 3 ? Ji0[3 * a + k] : Ji1[3 * a + k - 3]) * C[6 * k + b];
            JC[6 * a + b] = v;
        }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v += JC[6 * a + k] * (k < 3 ? Jj0[3 * b + k] : Jj1[3 * b + k - 3]);
            out[3 * a + b] = v;
        }
}

// hyp_ptr: n_hyp + 1 candidate offsets; tab_ptr: n_hyp + 1 offsets into tab, which holds per hypothesis and per lower block (i, j), j <= i, in
// the order (0,0) (1,0) (1,1) (2,0) ... four entries: S(a_i,a_j), S(a_i,b_j), S(b_i,a_j), S(b_i,b_j); c_ptr: n_hyp offsets into C_out;
// in: 18 doubles per candidate (k_gate_xyt's); n_slots: the blocks in cov.  d2: one prefix per candidate; bad[h]: 1.0 where a pivot was not
// positive (the prefixes are NaN from that candidate on), else 0.0; C_out (or null): the matrices, row-major, fully symmetric.
__global__ void __launch_bounds__(JG_T) k_gate_xyt_joint(int n_hyp, const int *__restrict__ hyp_ptr, const int *__restrict__ tab_ptr, const int *__restrict__ tab,
                                                         const long long *__restrict__ c_ptr, const double *__restrict__ in, int n_slots,
                                                         const double *__restrict__ cov, double *__restrict__ d2, double *__restrict__ bad,
                                                         double *__restrict__ C_out) {
    __shared__ double Cs[JG_N][JG_LD];
    __shared__ double Js[JG_MAX][18], Wi[JG_MAX][9], rs[JG_N], ys[JG_N];
    __shared__ double piv;
    const int h = blockIdx.x, tid = threadIdx.x;
    if (h >= n_hyp) return;
    const int c0 = hyp_ptr[h], m = hyp_ptr[h + 1] - c0, n = 3 * m;
    if (m < 1 || m > JG_MAX) return;
    if (tid < m) {
        const double *q = in + 18ll * (c0 + tid);
        factor_residual(true, q, q + 3, q + 6, Js[tid], Js[tid] + 9, rs + 3 * tid);
        const double *W = q + 9;                          // W^-1 by the adjugate, as k_gate_xyt (W was checked positive definite on the host)
        const double det = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
        const double wi[9] = { (W[4] * W[8] - W[5] * W[7]) / det, (W[2] * W[7] - W[1] * W[8]) / det, (W[1] * W[5] - W[2] * W[4]) / det,
                               (W[5] * W[6] - W[3] * W[8]) / det, (W[0] * W[8] - W[2] * W[6]) / det, (W[2] * W[3] - W[0] * W[5]) / det,
                               (W[3] * W[7] - W[4] * W[6]) / det, (W[1] * W[6] - W[0] * W[7]) / det, (W[0] * W[4] - W[1] * W[3]) / det };
#pragma unroll
        for (int k = 0; k < 9; k++) Wi[tid][k] = wi[k];
    }
    __syncthreads();
    const int *tb = tab + tab_ptr[h];
    for (int blk = tid; blk < m * (m + 1) / 2; blk += JG_T) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= blk) i++;
        const int j = blk - i * (i + 1) / 2;
        double C6[36], S[9];
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 4; e++) {                     // quarter e of C6 from its slot's quarter
            const int code = tb[4 * blk + e], slot = code >> 2, ro = (code & 2) ? 3 : 0, co = (code & 1) ? 3 : 0;
            ok = ok && slot >= 0 && slot < n_slots;
            const double *B = cov + 36ll * (ok ? slot : 0);
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y < 3; y++) C6[6 * ((e >> 1) * 3 + x) + (e & 1) * 3 + y] = ok ? B[6 * (ro + x) + co + y] : NAN;
        }
        if (i == j) {                                     // the candidate's own pair: k_gate_xyt's S
            xyt_joint_cov(Js[i], Js[i] + 9, C6, S);
#pragma unroll
            for (int k = 0; k < 9; k++) S[k] = S[k] + Wi[i][k];
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y <= x; y++) { Cs[3 * i + x][3 * i + y] = S[3 * x + y]; Cs[3 * i + y][3 * i + x] = S[3 * x + y]; }
        } else {
            xyt_cross_cov(Js[i], Js[i] + 9, C6, Js[j], Js[j] + 9, S);
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y < 3; y++) { Cs[3 * i + x][3 * j + y] = S[3 * x + y]; Cs[3 * j + y][3 * i + x] = S[3 * x + y]; }
        }
    }
    __syncthreads();
    if (C_out) {
        double *o = C_out + c_ptr[h];
        for (int e = tid; e < n * n; e += JG_T) o[e] = Cs[e / n][e % n];
        __syncthreads();                                  // (the factorisation overwrites the lower triangle)
    }
    // C = L L' in the lower triangle and y = L^-1 r, column by column; `done` = the columns whose pivot was positive
    int done = n;
    for (int c = 0; c < n; c++) {
        double v = 0.0;
        if (tid >= c && tid < n) {
            v = Cs[tid][c];
            for (int k = 0; k < c; k++) v -= Cs[tid][k] * Cs[c][k];
            if (tid == c) piv = v;
        }
        __syncthreads();
        const double p = piv;
        if (!(p > 0.0)) { done = c; break; }              // (uniform: every thread reads the same pivot)
        const double d = sqrt(p);
        if (tid > c && tid < n) Cs[tid][c] = v / d;
        if (tid == c) {
            Cs[c][c] = d;
            double t = rs[c];
            for (int k = 0; k < c; k++) t -= Cs[c][k] * ys[k];
            ys[c] = t / d;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            if (3 * j + 3 <= done) {
                for (int k = 0; k < 3; k++) acc += ys[3 * j + k] * ys[3 * j + k];
                d2[c0 + j] = acc;
            } else d2[c0 + j] = NAN;
        }
        bad[h] = done < n ? 1.0 : 0.0;
    }
}

}  // namespace asam
