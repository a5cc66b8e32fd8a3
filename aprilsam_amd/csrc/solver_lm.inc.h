// solver_lm.inc.h -- part of solver.hip.cpp (ONE translation unit), included from there, inside namespace asam.  Contents: the driver of
// aprilsam_amd_optimize_lm, Levenberg-Marquardt on the device (kernels in lm.hip.h).
//
// Set-up is resident_begin_impl's (pack, plan, upload).  One iteration = the numeric phase with its state update pointed at the trial
// buffer, then cost / model / norms / decide / commit, captured once as c.cap_lm and replayed; the host synchronises every check_every
// iterations and reads the status block k_lm_decide mirrors into pinned memory.  The end copies the states back as resident_end does and
// drops the retained factor (it was made at another point with another lambda).

void lm_opts_init(aprilsam_amd_lm_opts_t *o) {
    if (!o) return;
    o->max_iters = 50; o->check_every = 1;
    o->lambda0 = 1e-4; o->lambda_max = 1e16; o->eta = 0.0; o->ftol = 1e-10; o->xtol = 1e-10;
}

static const char *lm_bad_options(const aprilsam_amd_lm_opts_t *o) {
    if (o->max_iters < 1) return "max_iters must be >= 1";
    if (o->check_every < 1) return "check_every must be >= 1";
    if (!(o->lambda0 > 0) || !std::isfinite(o->lambda0)) return "lambda0 must be finite and > 0";
    if (!(o->lambda_max > 0) || std::isnan(o->lambda_max)) return "lambda_max must be > 0";
    if (!(o->eta >= 0 && o->eta < 1)) return "eta must lie in [0, 1)";
    if (!(o->ftol >= 0) || !std::isfinite(o->ftol)) return "ftol must be finite and >= 0";
    if (!(o->xtol >= 0) || !std::isfinite(o->xtol)) return "xtol must be finite and >= 0";
    return nullptr;
}

// F at st -> *out
static void lm_enqueue_cost(Context &c, GraphPack &gp, hipStream_t s, const double *st, double *out) {
    const int F = gp.F, T = std::max(F, 2 * gp.N);
    double *terms = c.d_lm_terms.p;
    enqueue_objective(gp, s, Convention::LM, st, terms);
    enqueue_reduce(REDUCE_SUM, s, F, terms, terms + T, out);
}
static void lm_enqueue_commit(Context &c, GraphPack &gp, hipStream_t s) {
    const int N = gp.N;
    hipLaunchKernelGGL(k_lm_commit, dim3((N + TPB - 1) / TPB), dim3(TPB), 0, s, N, (const LmScalars *)c.d_lm.p, c.d_lm_trial.p, (const double *)gp.d_dx.p,
                       gp.d_state.p, gp.d_lp.p, c.d_lm_hacc.p, c.d_lambda.p, c.d_bad.p);
}
// one LM iteration (DESIGN.md section 14, steps 1-5 and the decision)
static void lm_enqueue_iteration(Context &c, GraphPack &gp, hipStream_t s) {
    const int N = gp.N, F = gp.F, T = std::max(F, 2 * N);
    LmScalars *S = c.d_lm.p;
    double *terms = c.d_lm_terms.p, *parts = terms + T;
    NumericArgs trial; trial.st_dest = c.d_lm_trial.p;
    enqueue_numeric(c, gp, s, trial);      // select, linearise, factor, solve: x_t -> trial
    lm_enqueue_cost(c, gp, s, c.d_lm_trial.p, &S->Ft);
    hipLaunchKernelGGL(k_lm_model, dim3((F + TPB - 1) / TPB), dim3(TPB), 0, s, F, gp.d_fa.p, gp.d_fb.p, gp.d_z.p, gp.d_W.p, (const double *)gp.d_lp.p,
                       (const double *)gp.d_dx.p, terms);
    launch_gaussian(s, gp, k_lm_model_gaussian, (const double *)gp.d_lp.p, (const double *)gp.d_dx.p, terms);      // (their slots are null: h' (2 g - Lambda h) from the table)
    enqueue_reduce(REDUCE_SUM, s, F, terms, parts, &S->pred);
    hipLaunchKernelGGL(k_lm_norms, dim3((N + TPB - 1) / TPB), dim3(TPB), 0, s, N, (const double *)gp.d_dx.p, (const double *)gp.d_state.p, terms, terms + N);
    enqueue_reduce(REDUCE_SUM, s, N, terms, parts, &S->hh);
    enqueue_reduce(REDUCE_SUM, s, N, terms + N, parts, &S->xx);
    hipLaunchKernelGGL(k_lm_decide, dim3(1), dim3(64), 0, s, S, c.h_lm.p, (const int *)c.d_bad.p, c.d_lm_trace.p);
    lm_enqueue_commit(c, gp, s);
    HIPCHECK(hipGetLastError());
}
static void lm_run_iteration(Context &c, GraphPack &gp, hipStream_t s) {
    rewind_epoch(c, s, 1);
    if (!g_opt.use_graph) { lm_enqueue_iteration(c, gp, s); return; }
    const CaptureKey key = gp.capture_key({ (size_t)c.d_lm_trial.p, (size_t)c.d_lm_terms.p, (size_t)c.d_lm_trace.p, (size_t)c.d_lm.p, (size_t)gp.N, (size_t)gp.gc_gen });
    replay_captured(c, c.cap_lm, key, s, [&] { lm_enqueue_iteration(c, gp, s); });
}

// ---- the pieces of a run, shared with the stage driver of aprilsam_amd_optimize_gnc (solver_gnc.inc.h) --------------------------------
// refusals before anything is uploaded: the param keeps whatever it had.  0, or the code gate_refuse returned
static int lm_refuse_graph(const char *who, april_graph_t *g, april_graph_cholesky_param_t *param) {
    char msg[256];
    SlotLock lk(param, g);
    if (g_shard.find(param) != g_shard.end()) { snprintf(msg, sizeof msg, "%s: sharded params are not supported", who); return gate_refuse(ERR_UNSUPPORTED, msg); }
    GraphPack &gp = pack_for(g);
    pack_factors(gp, g);
    if (!gp.host_idx.empty()) { snprintf(msg, sizeof msg, "%s: the graph holds host-evaluated factors (foreign types): use april_graph_cholesky", who); return gate_refuse(-4, msg); }
    if (gp.n_asym > 0) {
        snprintf(msg, sizeof msg, "%s: a factor has an asymmetric information matrix (the reference-order step does not minimise the cost)", who);
        return gate_refuse(ERR_UNSUPPORTED, msg);
    }
    return 0;
}
// after resident_begin_impl: the run's buffers, state = l_point = x0, no step accepted yet
static void lm_enter(Context &c, GraphPack &gp, hipStream_t s, const aprilsam_amd_lm_opts_t *o) {
    const int N = gp.N, F = gp.F, T = std::max(F, 2 * N);
    set_small_attr();
    gp.mirror_sync = false; gp.lp_last_valid = false;
    c.d_lm_trial.need((size_t)3 * N); c.d_lm_hacc.need((size_t)3 * N);
    c.d_lm_terms.need((size_t)T + REDUCE_PARTS); c.d_lm_trace.need((size_t)4 * o->max_iters);
    c.d_lm.need(1); c.h_lm.need(1);
    HIPCHECK(hipMemcpyAsync(gp.d_lp.p, gp.d_state.p, (size_t)24 * N, hipMemcpyDeviceToDevice, s));          // state = l_point = x0
    HIPCHECK(hipMemsetAsync(c.d_lm_hacc.p, 0xff, (size_t)24 * N, s));                                     // (NaN: no step accepted yet)
    // d_lambda is about to hold the LM damping: whatever runs next on this param must rewrite it
    c.lambda_N = -1; c.lambda_val = -1;
    c.have_fact = false; c.fact_kind = FACT_NONE;
}
// the scalars of a run that starts at the current x (lambda0, nu = 2, counters 0), F(x) and the first commit; the stream is NOT synchronised.
// mirror: F(x) is copied into c.h_lm as well (valid once the stream has been synchronised, and not to be read before)
static void lm_enqueue_start(Context &c, GraphPack &gp, hipStream_t s, const aprilsam_amd_lm_opts_t *o, bool mirror = true) {
    LmScalars &h = *c.h_lm.p;
    h = LmScalars{};
    h.lambda = o->lambda0; h.nu = 2.0; h.eta = o->eta; h.ftol = o->ftol; h.xtol = o->xtol; h.lambda_max = o->lambda_max; h.max_iters = o->max_iters;
    HIPCHECK(hipMemcpyAsync(c.d_lm.p, c.h_lm.p, sizeof(LmScalars), hipMemcpyHostToDevice, s));
    lm_enqueue_cost(c, gp, s, gp.d_state.p, &c.d_lm.p->F);
    lm_enqueue_commit(c, gp, s);           // (accept_now = 0: trial = x0, d_lambda = lambda0, failure record cleared)
    if (mirror) HIPCHECK(hipMemcpyAsync(c.h_lm.p, c.d_lm.p, sizeof(LmScalars), hipMemcpyDeviceToHost, s));
}
// iterations until a stop test holds, the host synchronising every check_every of them
static void lm_iterate(Context &c, GraphPack &gp, hipStream_t s, const aprilsam_amd_lm_opts_t *o) {
    LmScalars &h = *c.h_lm.p;
    while (true) {
        // (status 0: fewer than max_iters iterations so far; the chunk never runs past the iterations still allowed)
        const int chunk = std::min(o->check_every, o->max_iters - h.iterations);
        for (int k = 0; k < chunk; k++) lm_run_iteration(c, gp, s);
        HIPCHECK(hipStreamSynchronize(s));
        if (h.status == LM_FAULT) {               // a dependency time-out: fails the call (ERR_DEP_TIMEOUT) as on every solver path
            memcpy(c.h_bad.p, h.fault, sizeof(h.fault));
            check_bad(c);
        }
        if (h.status != 0) break;
    }
}
// results: state = l_point = x*, delta_X = the last accepted h; returns april_graph_chi2 of x* (synchronises the stream)
static double lm_write_back(Context &c, GraphPack &gp, hipStream_t s, april_graph_t *g) {
    const int N = gp.N;
    HIPCHECK(hipMemcpyAsync(gp.h_state.p, gp.d_state.p, (size_t)24 * N, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(gp.h_dx.p, c.d_lm_hacc.p, (size_t)24 * N, hipMemcpyDeviceToHost, s));
    const double chi2 = device_chi2(gp);          // (synchronises the stream)
    memcpy(gp.h_lp.p, gp.h_state.p, (size_t)24 * N);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < N; i++) {
        april_graph_node_t *n = ns[i];
        memcpy(n->state, gp.h_state.p + (size_t)3 * i, 24);
        memcpy(n->l_point, gp.h_state.p + (size_t)3 * i, 24);
        const double *dx = gp.h_dx.p + (size_t)3 * i;
        if (!(std::isnan(dx[0]) || std::isnan(dx[1]) || std::isnan(dx[2]))) memcpy(n->delta_X, dx, 24);
    }
    return chi2;
}

static int optimize_lm_impl(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_lm_opts_t *o, aprilsam_amd_lm_report_t *report,
                            double *trace) {
    ensure_device();
    if (int rc = lm_refuse_graph("aprilsam_amd_optimize_lm", g, param)) return rc;
    if (int rc = resident_begin_impl(g, param)) return rc;        // pack, plan, upload (as the resident loop)
    SlotLock lk(param, g);
    Context &c = ctx_for(param);
    GraphPack &gp = pack_for(g);
    hipStream_t s = gp.stream;
    lm_enter(c, gp, s, o);
    lm_enqueue_start(c, gp, s, o);
    HIPCHECK(hipStreamSynchronize(s));
    LmScalars &h = *c.h_lm.p;
    const double F0 = h.F;
    lm_iterate(c, gp, s, o);
    std::vector<double> tr;
    if (trace && h.iterations > 0) {
        tr.resize((size_t)4 * h.iterations);
        HIPCHECK(hipMemcpy(tr.data(), c.d_lm_trace.p, tr.size() * 8, hipMemcpyDeviceToHost));      // (lm_iterate left the stream idle)
    }
    const double chi2 = lm_write_back(c, gp, s, g);
    if (trace && !tr.empty()) memcpy(trace, tr.data(), tr.size() * 8);
    report->status = h.status; report->iterations = h.iterations; report->accepted = h.accepted; report->rejected_not_spd = h.rejected_not_spd;
    report->F_initial = F0; report->F_final = h.F; report->chi2_final = chi2; report->lambda_final = h.lambda;
    return 0;
}

int optimize_lm(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_lm_opts_t *opts, aprilsam_amd_lm_report_t *report, double *trace) {
    const char *who = "aprilsam_amd_optimize_lm";
    char msg[256];
    if (!g || !param || !opts || !report) { snprintf(msg, sizeof msg, "%s: null argument", who); return gate_refuse(ERR_BAD_GRAPH, msg); }
    if (const char *why = lm_bad_options(opts)) { snprintf(msg, sizeof msg, "%s: bad options: %s", who, why); return gate_refuse(ERR_BAD_GRAPH, msg); }
    if (zsize(g->nodes) == 0 || zsize(g->factors) == 0) { snprintf(msg, sizeof msg, "%s: empty graph", who); return gate_refuse(-1, msg); }
    return guarded_rc(param, g, [&] { return optimize_lm_impl(g, param, opts, report, trace); });
}
