// jointgate.hip.h -- part of solver.hip.cpp (included after pathsolve.hip.h).  The frame of the joint measures over lists of at most JG_MAX
// entries -- a symmetric matrix of 3 x 3 blocks in LDS, factorised by columns, one value per leading block out -- and its first rider: joint
// compatibility gating of closure hypotheses (aprilsam_amd_gate_xyt_joint), the Mahalanobis distance of the stacked residual of a SET of
// candidate xyt measurements under their full joint innovation covariance, cross terms included.  The riders of the information measures:
// infomeasure.hip.h.  Host driver: solver_gating.inc.h.  DESIGN.md sections 29 and 33.
//
// k_block_chol<R> runs behind the path solves (pathsolve.hip.h): `cov` holds the 6 x 6 joint blocks k_path_gram formed (k_fix_cov applied),
// one per DISTINCT unordered node pair of the call.  One workgroup of one wave per list of m <= JG_MAX entries, n = 3 m rows:
//     R::setup      per entry, thread t the list's entry t (the riders over candidates: XytCand::setup)
//     R::block      C(i, j), one thread per lower 3 x 3 block, stored with its mirror image; what it reads of `cov` comes through the index
//                   table: entry = 4 slot + sub, sub picking the 3 x 3 quarter of the slot's block (1: rows 0..2 / columns 3..5, 2: the mirror
//                   quarter -- the same pair read the other way round --, 0 / 3: the diagonal quarters) (load_quarter)
//     C = L L'      by columns, thread t owning row t; thread c hands L_cc and row c to R::column
//     R::prefix     on thread 0, j ascending: the value of the list's first j + 1 entries; NaN from the first pivot that is not positive on
// JointGate:  r_i, J_ai, J_bi, W_i^-1 per candidate (factor_residual, xyt_info_inverse), four table entries per block,
//     C(i, j) = [J_ai J_bi] [[S(a_i,a_j) S(a_i,b_j)]; [S(b_i,a_j) S(b_i,b_j)]] [J_aj J_bj]'  (+ W_i^-1 on the diagonal),
//     y = L^-1 r in the column step, prefix j = sum of y_t^2 over t < 3 (j + 1).
// C and the riders' arrays stay in LDS.  C's leading dimension JG_LD is odd: thread t walks row t (ds_read_b64 at a stride of 2 JG_LD dwords,
// 32 lanes on 32 distinct bank pairs), the pivot row is one address for all lanes (a broadcast).  Every sum runs over k ascending in one
// thread, no atomics, no reduction whose shape depends on m: element (t, c) of L and what a rider makes of column c take the same operations
// whatever follows them, so a list cut to its first j entries reproduces prefix j bit for bit, and two calls give the same bits.  Plain
// vector stores to pinned memory.  The host promises 1 <= m <= JG_MAX and table entries inside cov; a broken table is not run (the guards
// return, a slot outside cov reads as NaN).
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

constexpr int JG_MAX = 16;       // entries per list (APRILSAM_AMD_JOINT_MAX, APRILSAM_AMD_SET_MAX)
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

// the 3 x 3 quarter the table entry `code` names, into out (leading dimension ld); ok: the entries so far lay inside cov -- NaN once one did not
__device__ __forceinline__ void load_quarter(int code, int n_slots, const double *__restrict__ cov, bool &ok, double *out, int ld) {
    const int slot = code >> 2, ro = (code & 2) ? 3 : 0, co = (code & 1) ? 3 : 0;
    ok = ok && slot >= 0 && slot < n_slots;
    const double *B = cov + 36ll * (ok ? slot : 0);
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) out[ld * x + y] = ok ? B[6 * (ro + x) + co + y] : NAN;
}

// C6 (6 x 6) from the four entries at tb: S(a_i,a_j), S(a_i,b_j), S(b_i,a_j), S(b_i,b_j)
__device__ __forceinline__ void load_c6(const int *__restrict__ tb, int n_slots, const double *__restrict__ cov, double *C6) {
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 4; e++) load_quarter(tb[e], n_slots, cov, ok, C6 + 18 * (e >> 1) + 3 * (e & 1), 6);
}

// What the riders over candidate xyt measurements share.  `in`: 18 doubles per candidate (state a, state b, z, W: k_gate_xyt's).  (A rider
// is aligned as a __shared__ array of its own would be: its members' sizes are multiples of 16 bytes, and the Jacobians go by ds_read_b128)
struct alignas(16) XytCand {
    static constexpr int PER = 4;                         // table entries per block
    double Js[JG_MAX][18], Wi[JG_MAX][9];
    // candidate t of the list: J_a, J_b and W^-1 into their places, the residual against z into r; returns det W
    __device__ __forceinline__ double setup(int t, const double *q, const double *z, double *r) {
        factor_residual(true, q, q + 3, z, Js[t], Js[t] + 9, r);
        double wi[9];
        const double det = xyt_info_inverse(q + 9, wi);   // (W was checked positive definite on the host)
#pragma unroll
        for (int k = 0; k < 9; k++) Wi[t][k] = wi[k];
        return det;
    }
    __device__ __forceinline__ void block(const int *__restrict__ tb, int i, int j, int n_slots, const double *__restrict__ cov, double *S) const {
        double C6[36];
        load_c6(tb, n_slots, cov, C6);
        if (i == j) {                                     // the candidate's own pair: k_gate_xyt's S
            xyt_joint_cov(Js[i], Js[i] + 9, C6, S);
#pragma unroll
            for (int k = 0; k < 9; k++) S[k] = S[k] + Wi[i][k];
        } else xyt_cross_cov(Js[i], Js[i] + 9, C6, Js[j], Js[j] + 9, S);
    }
};

// c_ptr: n_hyp offsets into C_out, which (if not null) receives the matrices, row-major, fully symmetric
struct JointGate : XytCand {
    double rs[JG_N], ys[JG_N];
    __device__ __forceinline__ void setup(int t, int at, const double *__restrict__ in) {
        const double *q = in + 18ll * at;
        XytCand::setup(t, q, q + 6, rs + 3 * t);
    }
    __device__ __forceinline__ void matrix(const double (*Cs)[JG_LD], int n, int h, const long long *__restrict__ c_ptr, double *__restrict__ C_out) const {
        if (!C_out) return;
        double *o = C_out + c_ptr[h];
        for (int e = threadIdx.x; e < n * n; e += JG_T) o[e] = Cs[e / n][e % n];
        __syncthreads();                                  // (the factorisation overwrites the lower triangle)
    }
    __device__ __forceinline__ void column(int c, double d, const double *Lc) {      // y_c of y = L^-1 r
        double t = rs[c];
        for (int k = 0; k < c; k++) t -= Lc[k] * ys[k];
        ys[c] = t / d;
    }
    __device__ __forceinline__ double prefix(int j, double *acc) const {
        for (int k = 0; k < 3; k++) acc[0] += ys[3 * j + k] * ys[3 * j + k];
        return acc[0];
    }
};

// hyp_ptr: n_hyp + 1 offsets of the lists' entries; tab_ptr: n_hyp + 1 offsets into tab, which holds per list and per lower block (i, j),
// j <= i, in the order (0,0) (1,0) (1,1) (2,0) ... R::PER entries; n_slots: the blocks in cov; in, c_ptr, C_out: the rider's (null where it
// has none).  out: one prefix per entry; bad[h]: 1.0 where a pivot was not positive (the prefixes are NaN from that entry on), else 0.0.
template <class R>
__global__ void __launch_bounds__(JG_T) k_block_chol(int n_hyp, const int *__restrict__ hyp_ptr, const int *__restrict__ tab_ptr, const int *__restrict__ tab,
                                                     int n_slots, const double *__restrict__ cov, double *__restrict__ out, double *__restrict__ bad,
                                                     const double *__restrict__ in, const long long *__restrict__ c_ptr, double *__restrict__ C_out) {
    __shared__ double Cs[JG_N][JG_LD];
    __shared__ R rd;
    __shared__ double piv;
    const int h = blockIdx.x, tid = threadIdx.x;
    if (h >= n_hyp) return;
    const int c0 = hyp_ptr[h], m = hyp_ptr[h + 1] - c0, n = 3 * m;
    if (m < 1 || m > JG_MAX) return;
    if (tid < m) rd.setup(tid, c0 + tid, in);
    __syncthreads();
    const int *tb = tab + tab_ptr[h];
    for (int blk = tid; blk < m * (m + 1) / 2; blk += JG_T) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= blk) i++;
        const int j = blk - i * (i + 1) / 2;
        double S[9];
        rd.block(tb + R::PER * blk, i, j, n_slots, cov, S);
        if (i == j) {
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y <= x; y++) { Cs[3 * i + x][3 * i + y] = S[3 * x + y]; Cs[3 * i + y][3 * i + x] = S[3 * x + y]; }
        } else {
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y < 3; y++) { Cs[3 * i + x][3 * j + y] = S[3 * x + y]; Cs[3 * j + y][3 * i + x] = S[3 * x + y]; }
        }
    }
    __syncthreads();
    rd.matrix(Cs, n, h, c_ptr, C_out);
    // C = L L' in the lower triangle, column by column; `done` = the columns whose pivot was positive
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
        if (tid == c) { Cs[c][c] = d; rd.column(c, d, Cs[c]); }
        __syncthreads();
    }
    if (tid == 0) {
        double acc[2] = { 0.0, 0.0 };                     // the rider's running sums
        for (int j = 0; j < m; j++) out[c0 + j] = 3 * j + 3 <= done ? rd.prefix(j, acc) : NAN;
        bad[h] = done < n ? 1.0 : 0.0;
    }
}

}  // namespace asam
