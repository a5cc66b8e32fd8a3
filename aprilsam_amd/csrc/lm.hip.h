// lm.hip.h -- part of solver.hip.cpp (included after kernels.hip.h and maxmix.hip.h, whose factor_residual / rtWr it uses).
// Levenberg-Marquardt optimisation on the device.  One LM iteration is the existing numeric phase with its state
// update pointed at a trial buffer (enqueue_numeric's st_dest), followed by the kernels below:
//   k_lm_cost                        per factor r^T W r at the trial states (no 0.5); the other families' terms replace theirs in place, each
//                                    from its own header -- enqueue_objective's LM convention (solver_launch.inc.h)
//   k_lm_model                       per factor delta^T W (2 r - delta), delta = J_a h_a + J_b h_b, at the l_points (= x)
//   k_lm_norms                       per node |h_i|^2 and |x_i|^2
//   (enqueue_reduce sums each array into its own LmScalars field: k_reduce, behind k_reduce_parts above REDUCE_SPLIT terms)
//   k_lm_decide                      one thread: accept / reject (Nielsen), lambda, nu, stop tests, latch, counters, trace row; a
//                                    dependency time-out latches LM_FAULT instead (the call fails with ERR_DEP_TIMEOUT)
//   k_lm_commit                      per node: x <- trial if accepted, d_lambda <- lambda, trial <- x, failure record cleared
// Every kernel is elementwise or single-thread: no cross-workgroup flag.
#pragma once

namespace asam {

// LM_FAULT (never reported): a multi-level launch of an iteration gave up waiting for a dependency flag -- a failure of the launch, not a
// property of the problem.  The record is kept in LmScalars::fault and the host fails the call with ERR_DEP_TIMEOUT (check_bad).
enum { LM_CONVERGED_F = 1, LM_CONVERGED_X = 2, LM_STALLED = 3, LM_MAX_ITERS = 4, LM_FAULT = 5 };

// the run's scalars: one copy on the device, a pinned mirror k_lm_decide writes after every live iteration
struct LmScalars {
    double F, Ft, pred, hh, xx;          // F(x), F(x_t), model decrease, |h|^2, |x|^2
    double lambda, nu;
    double eta, ftol, xtol, lambda_max;  // options
    int status, iterations, accepted, rejected_not_spd;
    int accept_now, max_iters;           // accept_now: the decision of the iteration in flight (k_lm_commit reads it)
    int fault[4];                        // the failure record of the iteration that timed out (LM_FAULT), as d_bad held it
};

// per factor r^T W r at st (k_chi2 without the 1/2 on xyt terms: the other convention of factor_term, kernels.hip.h)
__global__ void __launch_bounds__(TPB) k_lm_cost(int F, const int *__restrict__ fa, const int *__restrict__ fb, const double *__restrict__ Z,
                                                 const double *__restrict__ Wm, const double *__restrict__ st, double *__restrict__ out) {
    factor_term<false>(F, fa, fb, Z, Wm, st, out);
}

// per factor delta^T W (2 r - delta) at lp, delta = J_a h_a + J_b h_b (xytpos: J = I); h = dx in node order.  Z / Wm: the slots as the
// linearisation read them (max factors: the component selected at lp)
__global__ void __launch_bounds__(TPB) k_lm_model(int F, const int *__restrict__ fa, const int *__restrict__ fb, const double *__restrict__ Z,
                                                  const double *__restrict__ Wm, const double *__restrict__ lp, const double *__restrict__ dx,
                                                  double *__restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int a = fa[f], b = fb[f];
    if (a < 0) { out[f] = 0; return; }
    double w[9], z[3], J0[9], J1[9], r[3], pa[3], pb[3] = { 0, 0, 0 }, ha[3], hb[3] = { 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 9; k++) w[k] = Wm[(size_t)9 * f + k];
#pragma unroll
    for (int k = 0; k < 3; k++) { z[k] = Z[(size_t)3 * f + k]; pa[k] = lp[(size_t)3 * a + k]; ha[k] = dx[(size_t)3 * a + k]; }
    const bool binary = b >= 0;
    if (binary) {
#pragma unroll
        for (int k = 0; k < 3; k++) { pb[k] = lp[(size_t)3 * b + k]; hb[k] = dx[(size_t)3 * b + k]; }
    }
    factor_residual(binary, pa, pb, z, J0, J1, r);
    double d[3], u[3];
    if (binary) {
        double d0[3], d1[3];
        a_v(J0, ha, d0); a_v(J1, hb, d1);
#pragma unroll
        for (int i = 0; i < 3; i++) d[i] = d0[i] + d1[i];
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) d[i] = ha[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) u[i] = 2.0 * r[i] - d[i];
    double Wu[3];
    a_v(w, u, Wu);
    out[f] = d[0] * Wu[0] + d[1] * Wu[1] + d[2] * Wu[2];
}

// per node |h_i|^2 -> hh[i], |x_i|^2 -> xx[i]
__global__ void __launch_bounds__(TPB) k_lm_norms(int N, const double *__restrict__ dx, const double *__restrict__ st, double *__restrict__ hh,
                                                  double *__restrict__ xx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double h0 = dx[(size_t)3 * i], h1 = dx[(size_t)3 * i + 1], h2 = dx[(size_t)3 * i + 2];
    const double x0 = st[(size_t)3 * i], x1 = st[(size_t)3 * i + 1], x2 = st[(size_t)3 * i + 2];
    hh[i] = h0 * h0 + h1 * h1 + h2 * h2;
    xx[i] = x0 * x0 + x1 * x1 + x2 * x2;
}

// one thread: the decision of the iteration.  Once S->status is set (the latch) an iteration changes nothing.
__global__ void k_lm_decide(LmScalars *__restrict__ S, LmScalars *__restrict__ mirror, const int *__restrict__ bad, double *__restrict__ trace) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    S->accept_now = 0;
    if (bad[0] == 9 || bad[2] == 9) {             // dependency time-out (wait_flag): no decision, the run ends and the call fails --
        if (S->status != LM_FAULT) {              // also in an iteration the latch has made a no-op
            S->status = LM_FAULT;
            for (int k = 0; k < 4; k++) S->fault[k] = bad[k];
            *mirror = *S;
        }
        return;
    }
    if (S->status != 0) return;
    const bool not_spd = bad[0] != 0;
    const double F = S->F, Ft = S->Ft, pred = S->pred, lam = S->lambda;
    const bool rejected = not_spd || isnan(S->hh) || !isfinite(Ft);
    const double rho = (F - Ft) / pred;
    int status = 0, acc = 0;
    if (!rejected && !(pred > 0)) {
        status = LM_CONVERGED_F;                  // no decrease left in the model
    } else if (!rejected && rho > S->eta) {
        acc = 1;
        const double t = 2.0 * rho - 1.0;
        S->lambda = lam * fmax(1.0 / 3.0, 1.0 - t * t * t);
        S->nu = 2.0;
        S->F = Ft;
        S->accepted += 1;
        if (F - Ft <= S->ftol * fabs(F)) status = LM_CONVERGED_F;
        else if (sqrt(S->hh) <= S->xtol * (sqrt(S->xx) + S->xtol)) status = LM_CONVERGED_X;
    } else {
        S->lambda = lam * S->nu;
        S->nu = 2.0 * S->nu;
        if (not_spd) S->rejected_not_spd += 1;
    }
    const int it = S->iterations;
    if (it < S->max_iters) {
        double *row = trace + (size_t)4 * it;
        row[0] = Ft; row[1] = rho; row[2] = lam; row[3] = acc;
    }
    S->iterations = it + 1;
    S->accept_now = acc;
    if (status == 0 && S->lambda > S->lambda_max) status = LM_STALLED;
    if (status == 0 && S->iterations >= S->max_iters) status = LM_MAX_ITERS;
    S->status = status;
    *mirror = *S;
}

// per node: x <- trial when the step was accepted (state and l_point), h -> hacc; lambda -> every position of d_lambda; trial <- x
// (a NaN component of the next h leaves its node unwritten by the update); the failure record is cleared for the next iteration
__global__ void __launch_bounds__(TPB) k_lm_commit(int N, const LmScalars *__restrict__ S, double *__restrict__ trial, const double *__restrict__ dx,
                                                   double *__restrict__ st, double *__restrict__ lp, double *__restrict__ hacc,
                                                   double *__restrict__ lambda, int *__restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { bad[0] = 0; bad[1] = 0; bad[2] = 0; bad[3] = 0; }
    if (i >= N) return;
    const bool acc = S->accept_now != 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const size_t e = (size_t)3 * i + k;
        double x = st[e];
        if (acc) { x = trial[e]; st[e] = x; lp[e] = x; hacc[e] = dx[e]; }
        trial[e] = x;
    }
    lambda[i] = S->lambda;
}

}  // namespace asam
