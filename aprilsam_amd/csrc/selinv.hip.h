// selinv.hip.h -- marginal covariances from the retained factor: multifrontal selected inversion (Takahashi recurrences) over
// the assembly tree, root to leaves, and the extraction of the 3 x 3 / 6 x 6 blocks a caller asks for.  Host driver:
// solver_marginals.inc.h.  DESIGN.md section 11 has the recurrence and the memory layout.
//
// For a front with own columns S (s = 3 nsb) and struct rows U (u = 3 nub), factor columns [L_SS; L_US], Sigma = A^-1:
//     Linv    = L_SS^-1                                   (k_selinv_diag: 16 x 16 diagonal blocks, k_selinv_trinv: the rest)
//     X       = L_US Linv                                 (k_selinv_x)
//     Sig_US  = -Sig_UU X                                 (k_selinv_sus; Sig_UU gathered from the parent by k_selinv_gather)
//     Sig_SS  = Linv^T Linv - X^T Sig_US                  (k_selinv_sss)
// The Sigma pool has the front pool's layout (same offsets, leading dimension R); it holds the FULL symmetric C x C block
// Sig_FF of every front (both triangles: the children's gathers and the extraction read any element without a branch).
// Linv (ld = s rounded up to 16) and X (ld = u rounded up to 16) live in a per-level scratch buffer.
//
// Every output element is written by exactly one lane, from sums in a fixed order (the MFMA k loop): two runs on the same
// factor give the same bits.  No atomics, no flags: one launch per kernel and level.
#pragma once
#include <hip/hip_runtime.h>

namespace asam {

constexpr int SEL_T = 16;                  // tile edge (v_mfma_f64_16x16x4_f64)
constexpr int SEL_GATHER_PER_WG = 1024;    // elements of Sig_UU per gather workgroup (256 threads x 4)

struct SelFront {
    long long off;             // frontal array in the factor pool == Sigma block in the Sigma pool
    long long scr;             // Linv in the level's scratch (ld = round16(s)); X follows at scr + round16(s)^2 (ld = round16(u))
    int s, u, R;               // own columns, struct rows (scalars), leading dimension
    int parent;                // assembly-tree parent (-1: root)
    int rows_begin;            // struct rows (positions, ascending) at this offset of the int arena
    int first, nsb;            // first own position, own blocks
    int rel_begin;             // the struct rows' blocks inside the parent's row list (f_rel) at this offset of the int arena
};
static_assert(sizeof(SelFront) == 48, "SelFront layout");

__host__ __device__ inline int sel_round16(int v) { return (v + 15) & ~15; }

typedef double sel_d4 __attribute__((ext_vector_type(4)));

// One wave: acc += A[0:16, k_lo:k_hi] * B[k_lo:k_hi, 0:16] on the matrix cores.  a(i, k) / b(k, j) return the operand element
// (0 outside the matrix).  Lane l supplies A[l & 15][k + (l >> 4)] and B[k + (l >> 4)][l & 15]; the result is
// acc[r] = D[(l >> 4) + 4 r][l & 15].  The loads of 16 k-steps are issued before their MFMAs (one memory latency per 64 k).
template <class FA, class FB>
__device__ __forceinline__ sel_d4 sel_mma(FA a, FB b, int k_lo, int k_hi, sel_d4 acc) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    constexpr int U = 16;
    for (int k0 = k_lo; k0 < k_hi; k0 += 4 * U) {
        double x[U], y[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int k = k0 + 4 * q + l4;
            const bool ok = k < k_hi;
            x[q] = ok ? a(l15, k) : 0.0;
            y[q] = ok ? b(k, l15) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < U; q++)
            if (k0 + 4 * q < k_hi) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[q], y[q], acc, 0, 0, 0);      // (wave-uniform)
    }
    return acc;
}

// The frame of a one-wave-per-entry kernel (four waves per workgroup): the wave's entry among the launch's n, -1 for an idle wave ...
__device__ __forceinline__ int sel_wave(int n) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    return w < n ? w : -1;
}
// ... and sel_mma's result handed out element by element: f(row, col, acc[r]) for the lane's four elements of the tile at (i0, c0)
// that lie inside rows x cols, r ascending.
template <class F>
__device__ __forceinline__ void sel_tile_store(int i0, int c0, int rows, int cols, sel_d4 acc, F f) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = i0 + l4 + 4 * r, col = c0 + l15;
        if (row < rows && col < cols) f(row, col, acc[r]);
    }
}

// One wave: V = L_SS^-1 V (TRANS: L_SS^-T V) in place on nc <= 16 columns of s rows (column-major, leading dimension ld), row block
// by row block: the first block first, TRANS the last.  L_SS[r][k] = L[r + k R].  Block i0: T = V_i - (the solved blocks' part of
// row block i) V_solved (MFMA), then the 16 x 16 triangle on the diagonal by substitution, lane per column (T: the wave's own LDS
// tile).  The wave reads back what it wrote in the blocks before (the fence makes those stores visible to its loads).  What the
// two directions differ in: the block order, the k range of the product, the order of the substitution, and tri.
template <bool TRANS>
__device__ __forceinline__ void tile_trsm(const double *__restrict__ L, int R, int s, double *V, int ld, int nc, double (*T)[SEL_T + 1]) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    // element (r0 + r, k0 + k) of the triangle solved with: L_SS, TRANS its transpose
    auto tri = [&](int r0, int r, int k0, int k) { return TRANS ? L[(long long)(r0 + r) * R + k0 + k] : L[(long long)(k0 + k) * R + r0 + r]; };
    for (int i0 = TRANS ? ((s - 1) / SEL_T) * SEL_T : 0; TRANS ? i0 >= 0 : i0 < s; i0 += TRANS ? -SEL_T : SEL_T) {
        const int m = min(SEL_T, s - i0);
        const int k_lo = TRANS ? i0 + SEL_T : 0, k_hi = TRANS ? s : i0;      // the rows solved already
        sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
        if (k_lo < k_hi)
            acc = sel_mma([&](int i, int k) { return i0 + i < s ? tri(i0, i, 0, k) : 0.0; },
                          [&](int k, int c) { return c < nc ? V[(long long)c * ld + k] : 0.0; }, k_lo, k_hi, acc);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = l4 + 4 * r;
            T[row][l15] = (row < m && l15 < nc) ? V[(long long)l15 * ld + i0 + row] - acc[r] : 0.0;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (wave-private tile: the wave's own LDS operations are in order)
        __builtin_amdgcn_sched_barrier(0);
        if (lane < nc) {
            double x[SEL_T];
#pragma unroll
            for (int q = 0; q < SEL_T; q++) {
                const int r = TRANS ? SEL_T - 1 - q : q;       // the row solved q-th, after the rows k above it (TRANS: below it)
                double v = 0.0;
                if (r < m) {
                    v = T[r][lane];
#pragma unroll
                    for (int k = TRANS ? r + 1 : 0; k < (TRANS ? SEL_T : r); k++)
                        if (!TRANS || k < m) v -= tri(i0, r, i0, k) * x[k];
                    v = v / tri(i0, r, i0, r);
                }
                x[r] = v;
            }
#pragma unroll
            for (int r = 0; r < SEL_T; r++) if (r < m) V[(long long)lane * ld + i0 + r] = x[r];
        }
        __threadfence();
    }
}

// Sig_UU of every front of a level from its parent's Sig_FF: child struct row a is row 3 rel[a / 3] + a % 3 of the parent (the
// extend-add's map, read the other way).  One workgroup per (front, chunk of 1024 elements): ent = { front, chunk }.  Only the
// front's first u struct rows take part: the phantom rows the incremental path appends to its last tail front (zero rows of L)
// are not counted in u.
__global__ void __launch_bounds__(256) k_selinv_gather(const SelFront *__restrict__ fr, const int *__restrict__ rel, const int4 *__restrict__ ent,
                                                       double *__restrict__ sig) {
    const int4 e = ent[blockIdx.x];
    const SelFront F = fr[e.x], Pf = fr[F.parent];
    const int u = F.u;
    const int *rl = rel + F.rel_begin;
    double *dst = sig + F.off + (long long)F.s * F.R + F.s;
    const double *src = sig + Pf.off;
    for (int q = 0; q < SEL_GATHER_PER_WG / 256; q++) {
        const long long el = (long long)e.y * SEL_GATHER_PER_WG + q * 256 + threadIdx.x;
        if (el >= (long long)u * u) break;
        const int a = (int)(el % u), b = (int)(el / u);
        const int pa = 3 * rl[a / 3] + a % 3, pb = 3 * rl[b / 3] + b % 3;
        dst[(long long)b * F.R + a] = src[(long long)pb * Pf.R + pa];
    }
}

// Inverses of the 16 x 16 diagonal blocks of L_SS, into the diagonal blocks of Linv (zeros above the diagonal).  One wave per
// (front, block): ent = { front, block }; lane c < 16 computes column c by forward substitution.
__global__ void __launch_bounds__(256) k_selinv_diag(const SelFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                     double *__restrict__ scr) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), c = threadIdx.x & 63;
    if (w >= n || c >= SEL_T) return;
    const int4 e = ent[w];
    const SelFront F = fr[e.x];
    const int i0 = SEL_T * e.y, m = min(SEL_T, F.s - i0), ls = sel_round16(F.s);
    const double *L = pool + F.off + (long long)i0 * F.R + i0;          // L[r + k R] = L_SS[i0 + r][i0 + k]
    double *Li = scr + F.scr + (long long)i0 * ls + i0;
    double x[SEL_T];
#pragma unroll
    for (int r = 0; r < SEL_T; r++) {
        double v = 0.0;
        if (r < m && c < m) {
            if (r == c) v = 1.0 / L[r + (long long)r * F.R];
            else if (r > c) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < r; k++) if (k >= c) acc += L[r + (long long)k * F.R] * x[k];
                v = -acc / L[r + (long long)r * F.R];
            }
        }
        x[r] = v;
    }
    if (c < m)
#pragma unroll
        for (int r = 0; r < SEL_T; r++) if (r < m) Li[(long long)c * ls + r] = x[r];
}

// The rest of Linv, one 16-column block per wave (ent = { front, column block }), row block by row block:
// Linv_ij = -Linv_ii * sum_{k = j .. i-1} L_ik Linv_kj.  The wave reads back what it wrote in earlier row blocks.
__global__ void __launch_bounds__(256) k_selinv_trinv(const SelFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                      double *__restrict__ scr) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n) return;
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    const int4 e = ent[w];
    const SelFront F = fr[e.x];
    const int s = F.s, R = F.R, ls = sel_round16(s), jb = SEL_T * e.y;
    const double *L = pool + F.off;
    double *Li = scr + F.scr;
    for (int i0 = jb + SEL_T; i0 < s; i0 += SEL_T) {
        sel_d4 T = (sel_d4){ 0, 0, 0, 0 };
        T = sel_mma([&](int i, int k) { return i0 + i < s ? L[(long long)k * R + i0 + i] : 0.0; },
                    [&](int k, int c) { return jb + c < s ? Li[(long long)(jb + c) * ls + k] : 0.0; }, jb, i0, T);
        sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {            // B = T: register ks of a lane holds T[4 ks + l4][l15], the k-step's operand
            const int m = 4 * ks + l4;
            const double x = (i0 + m < s && i0 + l15 < s) ? Li[(long long)(i0 + m) * ls + i0 + l15] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, T[ks], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = i0 + l4 + 4 * r, col = jb + l15;
            if (row < s && col < s) Li[(long long)col * ls + row] = -acc[r];
        }
        __threadfence();                            // (the next row block's loads see these stores)
    }
}

// X = L_US Linv: ent = { front, row tile (of u), column tile (of s) }, one wave per 16 x 16 tile.
__global__ void __launch_bounds__(256) k_selinv_x(const SelFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ pool,
                                                  double *__restrict__ scr) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const int4 e = ent[w];
    const SelFront F = fr[e.x];
    const int s = F.s, u = F.u, R = F.R, ls = sel_round16(s), lu = sel_round16(u), i0 = SEL_T * e.y, j0 = SEL_T * e.z;
    const double *Lus = pool + F.off + s;
    const double *Li = scr + F.scr;
    double *X = scr + F.scr + (long long)ls * ls;
    sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
    acc = sel_mma([&](int i, int k) { return i0 + i < u ? Lus[(long long)k * R + i0 + i] : 0.0; },
                  [&](int k, int c) { return j0 + c < s ? Li[(long long)(j0 + c) * ls + k] : 0.0; }, j0, s, acc);
    sel_tile_store(i0, j0, u, s, acc, [&](int row, int col, double v) { X[(long long)col * lu + row] = v; });
}

// Sig_US = -Sig_UU X, stored twice (rows U / columns S and its transpose): ent = { front, row tile (of u), column tile (of s) }.
__global__ void __launch_bounds__(256) k_selinv_sus(const SelFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ scr,
                                                    double *__restrict__ sig) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const int4 e = ent[w];
    const SelFront F = fr[e.x];
    const int s = F.s, u = F.u, R = F.R, ls = sel_round16(s), lu = sel_round16(u), i0 = SEL_T * e.y, j0 = SEL_T * e.z;
    double *S = sig + F.off;
    const double *X = scr + F.scr + (long long)ls * ls;
    sel_d4 acc = (sel_d4){ 0, 0, 0, 0 };
    acc = sel_mma([&](int i, int k) { return i0 + i < u ? S[(long long)(s + k) * R + s + i0 + i] : 0.0; },
                  [&](int k, int c) { return j0 + c < s ? X[(long long)(j0 + c) * lu + k] : 0.0; }, 0, u, acc);
    sel_tile_store(i0, j0, u, s, acc, [&](int row, int col, double v) { S[(long long)col * R + s + row] = -v; S[(long long)(s + row) * R + col] = -v; });
}

// Sig_SS = Linv^T Linv - X^T Sig_US on the lower tiles (ent = { front, row tile, column tile }, row >= column), each element
// (a >= c) stored at (a, c) and (c, a).
__global__ void __launch_bounds__(256) k_selinv_sss(const SelFront *__restrict__ fr, const int4 *__restrict__ ent, int n, const double *__restrict__ scr,
                                                    double *__restrict__ sig) {
    const int w = sel_wave(n);
    if (w < 0) return;
    const int4 e = ent[w];
    const SelFront F = fr[e.x];
    const int s = F.s, u = F.u, R = F.R, ls = sel_round16(s), lu = sel_round16(u), i0 = SEL_T * e.y, j0 = SEL_T * e.z;
    double *S = sig + F.off;
    const double *Li = scr + F.scr;
    const double *X = Li + (long long)ls * ls;
    sel_d4 acc = (sel_d4){ 0, 0, 0, 0 }, acx = (sel_d4){ 0, 0, 0, 0 };
    acc = sel_mma([&](int i, int k) { return i0 + i < s ? Li[(long long)(i0 + i) * ls + k] : 0.0; },
                  [&](int k, int c) { return j0 + c < s ? Li[(long long)(j0 + c) * ls + k] : 0.0; }, i0, s, acc);
    if (u > 0)
        acx = sel_mma([&](int i, int k) { return i0 + i < s ? X[(long long)(i0 + i) * lu + k] : 0.0; },
                      [&](int k, int c) { return j0 + c < s ? S[(long long)(j0 + c) * R + s + k] : 0.0; }, 0, u, acx);
    sel_tile_store(i0, j0, s, s, acc - acx, [&](int row, int col, double v) { if (row >= col) { S[(long long)col * R + row] = v; S[(long long)row * R + col] = v; } });
}

// Requested blocks, straight into pinned host memory in node order and node coordinates (x, y, theta: the unknowns of dx).
// qb == null: the 3 x 3 diagonal block of node qa[p] (9 values per node); else the joint block of (qa[p], qb[p]) (36 values,
// row-major, a's unknowns first), read from the front that owns the earlier-eliminated of the two; all 36 values NaN when the
// later one is not among that front's rows (the pair is not on the pattern of L).  One thread per output value.  pos: node ->
// elimination position, pos_front: position -> owning front.
// scalar row of elimination position q in front F's row list (own rows, then the struct rows by binary search), -1 if absent.  Shared with
// k_factor_audit (audit.hip.h).
__device__ __forceinline__ int sel_local_row(const SelFront &F, const int *__restrict__ rows, int q) {
    if (q >= F.first && q < F.first + F.nsb) return 3 * (q - F.first);
    int lo = 0, hi = F.u / 3;
    const int *rw = rows + F.rows_begin;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (rw[mid] < q) lo = mid + 1; else hi = mid; }
    return lo < F.u / 3 && rw[lo] == q ? F.s + 3 * lo : -1;
}

__global__ void __launch_bounds__(256) k_marginal_extract(int n, const int *__restrict__ qa, const int *__restrict__ qb, const int *__restrict__ pos,
                                                          const int *__restrict__ pos_front, const SelFront *__restrict__ fr, const int *__restrict__ rows,
                                                          const double *__restrict__ sig, double *__restrict__ out) {
    const int per = qb ? 36 : 9;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)n * per) return;
    const int p = (int)(g / per), e = (int)(g % per);
    if (!qb) {
        const int pa = pos[qa[p]], t = pos_front[pa];
        const SelFront F = fr[t];
        const int la = 3 * (pa - F.first), r = e / 3, c = e % 3;
        out[g] = sig[F.off + (long long)(la + c) * F.R + la + r];
        return;
    }
    const int pa = pos[qa[p]], pb = pos[qb[p]];
    const int t = pos_front[min(pa, pb)];
    const SelFront F = fr[t];
    const int la = sel_local_row(F, rows, pa), lb = sel_local_row(F, rows, pb);      // (the pair is on the pattern or it is not: one decision for all 36 values)
    const int r = e / 6, c = e % 6;
    const int lr = r < 3 ? la : lb, lc = c < 3 ? la : lb;
    out[g] = (la < 0 || lb < 0) ? __builtin_nan("") : sig[F.off + (long long)(lc + c % 3) * F.R + lr + r % 3];
}

}  // namespace asam
