// infomeasure.hip.h -- part of solver.hip.cpp (included after jointgate.hip.h).  Information measures from the retained factor: the
// log-determinant of the factorised system (aprilsam_amd_logdet), of the joint marginal covariance of node sets (aprilsam_amd_logdet_sets)
// and of I + W H Sigma H' of candidate xyt measurements (aprilsam_amd_info_gain_xyt).  Host driver: solver_info.inc.h, launchers:
// launch_info, launch_block_chol (solver_launch.inc.h).  DESIGN.md section 32.  All values are natural logarithms.
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
// The set and gain measures ride jointgate.hip.h's frame (k_block_chol<R>, behind the path solves; one wave per set / hypothesis, the matrix
// of n <= 48 rows in LDS, built from `cov` through the index table, C = L L' by columns).  Thread c keeps L_cc; thread 0 adds 2 log(L_cc)
// over c ascending: the value after column 3 j + 2 is prefix j.
//     SetLogdet   no set-up; one table entry per lower block (i, j): the 3 x 3 block S(node_i, node_j) as it lies in its slot
//     InfoGain    the joint gate's candidates, blocks and four entries per block (XytCand; the Jacobians of an xyt factor do not depend on z:
//                 the residual is taken against z = 0 and dropped), ln det W_i from the adjugate's det; prefix j = 0.5 (sum 2 log L_cc + sum ln det W_i)
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

constexpr int LD_CHUNK = 768;    // own columns per wave: 12 per lane; a multiple of 3 and of 64 (M3500's root: 1 chunk, a 12 645-column separator: 17)
constexpr int LD_SUM_T = 256;
constexpr int IM_SET_MAX = JG_MAX;      // nodes per set (APRILSAM_AMD_SET_MAX): the matrix is the frame's size

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

// the diagonal of L and its running sum of 2 log(L_cc)
struct alignas(16) LogdetDiag {
    double ld[JG_N];
    __device__ __forceinline__ void matrix(const double (*)[JG_LD], int, int, const long long *, double *) const {}
    __device__ __forceinline__ void column(int c, double d, const double *) { ld[c] = d; }
    __device__ __forceinline__ double prefix(int j, double *acc) const {
        for (int k = 0; k < 3; k++) acc[0] += 2.0 * log(ld[3 * j + k]);
        return acc[0];
    }
};

struct SetLogdet : LogdetDiag {
    static constexpr int PER = 1;
    __device__ __forceinline__ void setup(int, int, const double *) {}
    __device__ __forceinline__ void block(const int *__restrict__ tb, int, int, int n_slots, const double *__restrict__ cov, double *S) const {
        bool ok = true;
        load_quarter(tb[0], n_slots, cov, ok, S, 3);
    }
};

// in: 18 doubles per candidate (state a, state b, 3 unused, W)
struct InfoGain : XytCand, LogdetDiag {
    double lw[JG_MAX];
    __device__ __forceinline__ void setup(int t, int at, const double *__restrict__ in) {
        const double z0[3] = { 0.0, 0.0, 0.0 };
        double r[3];
        lw[t] = log(XytCand::setup(t, in + 18ll * at, z0, r));
    }
    __device__ __forceinline__ double prefix(int j, double *acc) const {
        const double ld2 = LogdetDiag::prefix(j, acc);
        acc[1] += lw[j];
        return 0.5 * (ld2 + acc[1]);
    }
};

}  // namespace asam
