// chordal.hip.h -- part of solver.hip.cpp (included after kernels.hip.h, whose TPB it uses).
// Chordal initialisation of the poses: two linear least-squares problems on the graph's own sparsity pattern,
// solved by the existing assembly, factorisation and back substitution.  Only what fills the contribution slots is new:
//   k_chordal_rot      per factor: stage 1, unknown u_i = (cos, sin) of pose i          -> the slots k_linearize fills
//   k_chordal_heading  per pose:   theta = atan2(s, c) of the stage-1 solution, |u|^2, degenerate flag
//   k_chordal_trans    per factor: stage 2, unknown t_i with the headings held fixed     -> the same slots
//   k_chordal_commit   per pose:   state = l_point = (t, theta)
// (min |u|^2 is the min op of the one reducer, k_chordal_min / k_chordal_min_parts in kernels.hip.h: one stage up to REDUCE_SPLIT poses)
// The third unknown of every pose is padding: a contributing factor writes 1.0 into element [2][2] of its diagonal blocks and zeros into
// the rest of the third row and column, so the padded unknown comes out exactly 0 and the 2-unknown system is otherwise unchanged.  A factor
// that fails a stage's condition writes zeros everywhere.  Every kernel is elementwise or a reduction of its own: no cross-workgroup flag.
#pragma once

namespace asam {

// where a launch takes factor i's data from: the packed slot itself (flist == null: f = i, z and W of f), the unweighted W of robust
// factor i (flist = rb_f, zsel = rb_f, wsel == null: W of row i), or the component the host chose for max factor i (zsel = wsel = it)
struct ChordalSrc { const int *flist, *zsel, *wsel; const double *Z, *Wm; };

// the six slots of factor f: Haa / Hab / Hbb (2 x 2, rows a, columns b for Hab), ga / gb (2), `on`: the factor contributes
__device__ __forceinline__ void chordal_store(int f, bool binary, bool on, const double *Haa, const double *Hab, const double *Hbb, const double *ga,
                                              const double *gb, const unsigned char *__restrict__ swp, const int *__restrict__ slot_blk,
                                              const int *__restrict__ slot_rhs, double *__restrict__ Hc) {
    const double pad = on ? 1.0 : 0.0;
    double *o = Hc + (size_t)slot_blk[3 * f] * 9;
    o[0] = Haa[0]; o[1] = Haa[1]; o[2] = 0; o[3] = Haa[1]; o[4] = Haa[3]; o[5] = 0; o[6] = 0; o[7] = 0; o[8] = pad;
    double *go = Hc + (size_t)slot_rhs[2 * f] * 9;
    go[0] = ga[0]; go[1] = ga[1]; go[2] = 0;
    if (!binary) return;
    const bool s = swp[f] & 1;          // final orientation: rows = the endpoint eliminated later (k_linearize's rule)
    double *o1 = Hc + (size_t)slot_blk[3 * f + 1] * 9, *o2 = Hc + (size_t)slot_blk[3 * f + 2] * 9;
    o1[0] = Hab[0]; o1[1] = s ? Hab[2] : Hab[1]; o1[2] = 0; o1[3] = s ? Hab[1] : Hab[2]; o1[4] = Hab[3]; o1[5] = 0; o1[6] = 0; o1[7] = 0; o1[8] = 0;
    o2[0] = Hbb[0]; o2[1] = Hbb[1]; o2[2] = 0; o2[3] = Hbb[1]; o2[4] = Hbb[3]; o2[5] = 0; o2[6] = 0; o2[7] = 0; o2[8] = pad;
    double *g1 = Hc + (size_t)slot_rhs[2 * f + 1] * 9;
    g1[0] = gb[0]; g1[1] = gb[1]; g1[2] = 0;
}

// stage 1, one thread per factor: xyt  w |R(z_theta) u_a - u_b|^2,  prior  w |u_a - (cos z_theta, sin z_theta)|^2,  w = W[2][2] > 0.
// The first launch of a stage (bad / epoch given) clears the failure record and advances the step counter as k_linearize does.
__global__ void __launch_bounds__(TPB) k_chordal_rot(int n, ChordalSrc src, const int *__restrict__ fa, const int *__restrict__ fb,
                                                     const unsigned char *__restrict__ swp, const int *__restrict__ slot_blk,
                                                     const int *__restrict__ slot_rhs, double *__restrict__ Hc, int *__restrict__ bad,
                                                     int *__restrict__ epoch) {
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) { bad[0] = 0; bad[1] = 0; bad[2] = 0; bad[3] = 0; }
    if (epoch && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(epoch, 1);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = src.flist ? src.flist[i] : i;
    const int a = fa[f], b = fb[f];
    if (a < 0) return;
    const size_t zi = src.zsel ? src.zsel[i] : i, wi = src.wsel ? src.wsel[i] : i;
    const double w = src.Wm[9 * wi + 8], zt = src.Z[3 * zi + 2];
    const bool on = w > 0;
    double Hd[4] = { 0, 0, 0, 0 }, Hab[4] = { 0, 0, 0, 0 }, ga[2] = { 0, 0 }, gb[2] = { 0, 0 };
    if (on) {
        double sn, cs;
        sincos(zt, &sn, &cs);
        Hd[0] = w; Hd[3] = w;
        if (b >= 0) { Hab[0] = -w * cs; Hab[1] = -w * sn; Hab[2] = w * sn; Hab[3] = -w * cs; }      // -w R(z_theta)^T
        else { ga[0] = w * cs; ga[1] = w * sn; }
    }
    chordal_store(f, b >= 0, on, Hd, Hab, Hd, ga, gb, swp, slot_blk, slot_rhs, Hc);
}

// per pose: the stage-1 solution (node order, 3 per pose) -> theta, |u|^2 and the degenerate flag (1.0 / 0.0: k_reduce counts them).
// A pose with |u|^2 == 0 or a non-finite component keeps its incoming heading; its |u|^2 is reported as 0
__global__ void __launch_bounds__(TPB) k_chordal_heading(int N, const double *__restrict__ u, const double *__restrict__ st, double *__restrict__ theta,
                                                         double *__restrict__ norm2, double *__restrict__ degen) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double c = u[(size_t)3 * i], s = u[(size_t)3 * i + 1];
    const double n2 = c * c + s * s;
    const bool ok = isfinite(c) && isfinite(s) && isfinite(n2) && n2 > 0;
    theta[i] = ok ? atan2(s, c) : st[(size_t)3 * i + 2];
    norm2[i] = ok ? n2 : 0.0;
    degen[i] = ok ? 0.0 : 1.0;
}

// stage 2, one thread per factor, headings fixed: xyt  |R(theta_a)^T (t_b - t_a) - z_xy|^2_Wxy,  prior  |t_a - z_xy|^2_Wxy, for
// W[0][0] > 0 and det Wxy > 0.  M = R_a Wxy R_a^T is formed once and its upper triangle mirrored: the system is symmetric to the bit
__global__ void __launch_bounds__(TPB) k_chordal_trans(int n, ChordalSrc src, const int *__restrict__ fa, const int *__restrict__ fb,
                                                       const double *__restrict__ theta, const unsigned char *__restrict__ swp,
                                                       const int *__restrict__ slot_blk, const int *__restrict__ slot_rhs, double *__restrict__ Hc,
                                                       int *__restrict__ bad, int *__restrict__ epoch) {
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) { bad[0] = 0; bad[1] = 0; bad[2] = 0; bad[3] = 0; }
    if (epoch && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(epoch, 1);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = src.flist ? src.flist[i] : i;
    const int a = fa[f], b = fb[f];
    if (a < 0) return;
    const size_t zi = src.zsel ? src.zsel[i] : i, wi = src.wsel ? src.wsel[i] : i;
    const double w00 = src.Wm[9 * wi], w01 = src.Wm[9 * wi + 1], w11 = src.Wm[9 * wi + 4];
    const double z0 = src.Z[3 * zi], z1 = src.Z[3 * zi + 1];
    const bool on = w00 > 0 && w00 * w11 - w01 * w01 > 0;
    double M[4] = { 0, 0, 0, 0 }, Mn[4] = { 0, 0, 0, 0 }, ga[2] = { 0, 0 }, gb[2] = { 0, 0 };
    if (on) {
        const double v0 = w00 * z0 + w01 * z1, v1 = w01 * z0 + w11 * z1;      // Wxy z_xy
        if (b >= 0) {
            double sn, cs;
            sincos(theta[a], &sn, &cs);
            // R W R^T with R = [c -s; s c]
            const double p00 = cs * w00 - sn * w01, p01 = cs * w01 - sn * w11, p10 = sn * w00 + cs * w01, p11 = sn * w01 + cs * w11;      // R Wxy
            M[0] = p00 * cs - p01 * sn; M[1] = p00 * sn + p01 * cs; M[3] = p10 * sn + p11 * cs; M[2] = M[1];
            Mn[0] = -M[0]; Mn[1] = -M[1]; Mn[2] = -M[1]; Mn[3] = -M[3];
            const double r0 = cs * v0 - sn * v1, r1 = sn * v0 + cs * v1;          // R_a Wxy z_xy
            ga[0] = -r0; ga[1] = -r1; gb[0] = r0; gb[1] = r1;
        } else {
            M[0] = w00; M[1] = w01; M[2] = w01; M[3] = w11;
            ga[0] = v0; ga[1] = v1;
        }
    }
    chordal_store(f, b >= 0, on, M, Mn, M, ga, gb, swp, slot_blk, slot_rhs, Hc);
}

// per pose, after both stages succeeded: state = l_point = (t, theta); t == null (headings only): positions keep their incoming values
__global__ void __launch_bounds__(TPB) k_chordal_commit(int N, const double *__restrict__ t, const double *__restrict__ theta, double *__restrict__ st,
                                                        double *__restrict__ lp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const size_t e = (size_t)3 * i;
    const double x = t ? t[e] : st[e], y = t ? t[e + 1] : st[e + 1], th = theta[i];
    st[e] = x; st[e + 1] = y; st[e + 2] = th;
    lp[e] = x; lp[e + 1] = y; lp[e + 2] = th;
}

}  // namespace asam
