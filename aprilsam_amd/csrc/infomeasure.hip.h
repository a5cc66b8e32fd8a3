// infomeasure.hip.h -- part of solver.hip.cpp (included after jointgate.hip.h).  Information measures from the retained factor: the
// log-determinant of the factorised system (aprilsam_amd_logdet), of the joint marginal covariance of node sets (aprilsam_amd_logdet_sets)
// and of I + W H Sigma H' of candidate xyt measurements (aprilsam_amd_info_gain_xyt).  Host driver: solver_info.inc.h, launcher:
// launch_info (solver_launch.inc.h).  DESIGN.md section 32.  All values are natural logarithms.
//
// ln det A = 2 sum ln L_jj over the own columns of every front.  L_jj of own column j of a front lies at pool[off + j (R + 1)]: the element
// tile_trsm (selinv.hip.h; k_path_trsm, k_ts_trsm) divides by, tri(i0, r, i0, r) = L[(i0 + r) R + i0 + r].  The inverse diagonal blocks the
// big fronts keep for the solver's own back substitution are another buffer and are not read.
//     k_logdet_partial   one wave per entry = (front, chunk of LD_CHUNK own columns): lane l takes columns l, l + 64, ... of the chunk,
//                        ascending, sums log(L_jj) and counts the entries that are not positive and finite; a fixed xor butterfly
//     k_logdet_sum       one workgroup: thread t adds the partials of its contiguous segment in index order, thread 0 the 256 segment
//                        sums in order; out[0] = 2 sum, out[1] = the count (pinned memory)
// The entries are made from the view alone (fronts ascending, chunks ascending): options that move offsets or reorder work lists give the
// same bits.  Plain loads, vector stores, no atomics, no flags.
//
// k_logdet_blocks runs behind the path solves in k_gate_xyt_joint's place: one workgroup of one wave per set / hypothesis, the matrix
// (n <= 48) in LDS with jointgate.hip.h's odd leading dimension, built from `cov` through the same index table (entry = 4 slot + quarter):
//     sets (in == null)   one entry per lower block (i, j): the 3 x 3 block S(node_i, node_j)
//     gain                four entries per lower block, J_ai, J_bi, W_i^-1 and C(i, j) exactly as k_gate_xyt_joint forms them (the Jacobians of
//                         an xyt factor do not depend on z: the residual is taken against z = 0 and dropped); ln det W_i from the adjugate's det
// then C = L L' by columns, thread t owning row t, and thread 0 adds 2 log(L_cc) over c ascending: the value after column 3 j + 2 is prefix
// j, and takes the same operations whatever follows it -- a set cut to its first j nodes reproduces prefix j bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

constexpr int LD_CHUNK = 768;    // own columns per wave: 12 per lane; a multiple of 3 and of 64 (M3500's root: 1 chunk, a 12 645-column separator: 17)
constexpr int LD_SUM_T = 256;
constexpr int IM_SET_MAX = JG_MAX;      // nodes per set (APRILSAM_AMD_SET_MAX): the matrix is k_gate_xyt_joint's size

struct LdEnt { long long at; int stride, n; };          // the chunk's first diagonal element in the pool, R + 1, its columns
static_assert(sizeof(LdEnt) == 16, "LdEnt layout");

__global__ void __launch_bounds__(256) k_logdet_partial(const LdEnt *__restrict__ ent, int n, const double *__restrict__ pool, double *__restrict__ part,
                                                        int *__restrict__ nbad) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const LdEnt e = ent[w];
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    int bad = 0;
    if (e.n <= LD_CHUNK)                                    // (the host promises it; a broken table is not read)
        for (int j = lane; j < e.n; j += 64) {
            const double d = pool[e.at + (long long)j * e.stride];
            if (d > 0.0 && d < INFINITY) acc += log(d);
            else bad++;
        }
    else bad = 1;
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) { acc += __shfl_xor(acc, st, 64); bad += __shfl_xor(bad, st, 64); }
    if (lane == 0) { part[w] = acc; nbad[w] = bad; }
}

__global__ void __launch_bounds__(LD_SUM_T) k_logdet_sum(int n, const double *__restrict__ part, const int *__restrict__ nbad, double *__restrict__ out) {
    __shared__ double sd[LD_SUM_T];
    __shared__ int sb[LD_SUM_T];
    const int tid = threadIdx.x, seg = (n + LD_SUM_T - 1) / LD_SUM_T;
    double acc = 0.0;
    int bad = 0;
    for (int i = tid * seg; i < min(n, (tid + 1) * seg); i++) { acc += part[i]; bad += nbad[i]; }
    sd[tid] = acc; sb[tid] = bad;
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < LD_SUM_T; t++) { acc += sd[t]; bad += sb[t]; }
        out[0] = 2.0 * acc;
        out[1] = (double)bad;
    }
}

// hyp_ptr: n_hyp + 1 offsets of the sets' nodes / the hypotheses' candidates; tab_ptr: n_hyp + 1 offsets into tab, which holds per set and
// lower block (i, j), j <= i, in the order (0,0) (1,0) (1,1) (2,0) ... one entry (sets) or k_gate_xyt_joint's four (gain); in: null (sets)
// or 18 doubles per candidate (state a, state b, 3 unused, W); n_slots: the blocks in cov.  out: one prefix per node / candidate (NaN from
// the first pivot that was not positive on); bad[h]: 1.0 for such a set, else 0.0.
__global__ void __launch_bounds__(JG_T) k_logdet_blocks(int n_hyp, const int *__restrict__ hyp_ptr, const int *__restrict__ tab_ptr, const int *__restrict__ tab,
                                                        const double *__restrict__ in, int n_slots, const double *__restrict__ cov,
                                                        double *__restrict__ out, double *__restrict__ bad) {
    __shared__ double Cs[JG_N][JG_LD];
    __shared__ double Js[JG_MAX][18], Wi[JG_MAX][9], lw[JG_MAX], ld[JG_N];
    __shared__ double piv;
    const int h = blockIdx.x, tid = threadIdx.x;
    if (h >= n_hyp) return;
    const int c0 = hyp_ptr[h], m = hyp_ptr[h + 1] - c0, n = 3 * m;
    if (m < 1 || m > JG_MAX) return;
    const bool gain = in != nullptr;
    if (gain && tid < m) {
        const double *q = in + 18ll * (c0 + tid);
        const double z0[3] = { 0.0, 0.0, 0.0 };
        double r[3];
        factor_residual(true, q, q + 3, z0, Js[tid], Js[tid] + 9, r);
        const double *W = q + 9;                          // W^-1 by the adjugate, as k_gate_xyt_joint (W was checked positive definite on the host)
        const double det = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
        const double wi[9] = { (W[4] * W[8] - W[5] * W[7]) / det, (W[2] * W[7] - W[1] * W[8]) / det, (W[1] * W[5] - W[2] * W[4]) / det,
                               (W[5] * W[6] - W[3] * W[8]) / det, (W[0] * W[8] - W[2] * W[6]) / det, (W[2] * W[3] - W[0] * W[5]) / det,
                               (W[3] * W[7] - W[4] * W[6]) / det, (W[1] * W[6] - W[0] * W[7]) / det, (W[0] * W[4] - W[1] * W[3]) / det };
#pragma unroll
        for (int k = 0; k < 9; k++) Wi[tid][k] = wi[k];
        lw[tid] = log(det);
    }
    __syncthreads();
    const int *tb = tab + tab_ptr[h];
    for (int blk = tid; blk < m * (m + 1) / 2; blk += JG_T) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= blk) i++;
        const int j = blk - i * (i + 1) / 2;
        double S[9];
        if (!gain) {                                      // the block S(node_i, node_j) as it lies in its slot
            const int code = tb[blk], slot = code >> 2, ro = (code & 2) ? 3 : 0, co = (code & 1) ? 3 : 0;
            const bool ok = slot >= 0 && slot < n_slots;
            const double *B = cov + 36ll * (ok ? slot : 0);
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y < 3; y++) S[3 * x + y] = ok ? B[6 * (ro + x) + co + y] : NAN;
        } else {
            double C6[36];
            bool ok = true;
#pragma unroll
            for (int e = 0; e < 4; e++) {                 // quarter e of C6 from its slot's quarter
                const int code = tb[4 * blk + e], slot = code >> 2, ro = (code & 2) ? 3 : 0, co = (code & 1) ? 3 : 0;
                ok = ok && slot >= 0 && slot < n_slots;
                const double *B = cov + 36ll * (ok ? slot : 0);
#pragma unroll
                for (int x = 0; x < 3; x++)
#pragma unroll
                    for (int y = 0; y < 3; y++) C6[6 * ((e >> 1) * 3 + x) + (e & 1) * 3 + y] = ok ? B[6 * (ro + x) + co + y] : NAN;
            }
            if (i == j) {
                xyt_joint_cov(Js[i], Js[i] + 9, C6, S);
#pragma unroll
                for (int k = 0; k < 9; k++) S[k] = S[k] + Wi[i][k];
            } else xyt_cross_cov(Js[i], Js[i] + 9, C6, Js[j], Js[j] + 9, S);
        }
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
        if (tid == c) { Cs[c][c] = d; ld[c] = d; }
        __syncthreads();
    }
    if (tid == 0) {
        double acc = 0.0, accw = 0.0;
        for (int j = 0; j < m; j++) {
            if (3 * j + 3 <= done) {
                for (int k = 0; k < 3; k++) acc += 2.0 * log(ld[3 * j + k]);
                if (gain) { accw += lw[j]; out[c0 + j] = 0.5 * (acc + accw); }
                else out[c0 + j] = acc;
            } else out[c0 + j] = NAN;
        }
        bad[h] = done < n ? 1.0 : 0.0;
    }
}

}  // namespace asam
