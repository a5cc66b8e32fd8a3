// solver_gnc.inc.h -- part of solver.hip.cpp (ONE translation unit), included from there after solver_lm.inc.h, inside namespace asam.
// Contents: the stage driver of aprilsam_amd_optimize_gnc, graduated non-convexity (kernels in gnc.hip.h).
//
// Set-up is optimize_lm's (solver_lm.inc.h: lm_refuse_graph, resident_begin_impl, lm_enter).  The candidates' table goes to the device
// once; from then until the call returns gp.gc_n > 0, which makes every linearisation weight them (enqueue_gnc_weight) and every
// objective of the LM convention count rho_mu for them (enqueue_objective).  A stage = k_gnc_set_mu, lm_enqueue_start, lm_iterate: the captured LM iteration is
// the same graph for every stage, mu being read from device memory.  The host synchronises once for s_max, once per check_every
// iterations, and for TLS once per stage (the "not all binary" flag); the per-stage entry objectives stay on the device until the end.

void gnc_opts_init(aprilsam_amd_gnc_opts_t *o) {
    if (!o) return;
    o->loss = APRILSAM_AMD_GNC_GM; o->c = sqrt(16.27); o->mu_step = 1.4; o->max_stages = 100;
    lm_opts_init(&o->lm);
    o->lm.max_iters = 10;
}

static const char *gnc_bad_options(const aprilsam_amd_gnc_opts_t *o) {
    if (o->loss != APRILSAM_AMD_GNC_GM && o->loss != APRILSAM_AMD_GNC_TLS) return "loss must be APRILSAM_AMD_GNC_GM or APRILSAM_AMD_GNC_TLS";
    if (!(o->c > 0) || !std::isfinite(o->c)) return "c must be finite and > 0";
    if (!(o->mu_step > 1) || !std::isfinite(o->mu_step)) return "mu_step must be finite and > 1";
    if (o->max_stages < 1) return "max_stages must be >= 1";
    return lm_bad_options(&o->lm);
}

static int optimize_gnc_impl(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_gnc_opts_t *o, int n, const int *cand,
                             aprilsam_amd_gnc_report_t *report, double *weights, double *stage_trace) {
    ensure_device();
    if (int rc = lm_refuse_graph("aprilsam_amd_optimize_gnc", g, param)) return rc;
    if (int rc = resident_begin_impl(g, param)) return rc;        // pack, plan, upload (as the resident loop)
    SlotLock lk(param, g);
    Context &c = ctx_for(param);
    GraphPack &gp = pack_for(g);
    hipStream_t s = gp.stream;
    const bool tls = o->loss == APRILSAM_AMD_GNC_TLS;
    const double cc = o->c * o->c;
    const int S = o->max_stages;
    // device: out = [values n | inlier flags n | parts REDUCE_PARTS | s_max, flag | entry objective per stage]; pinned staging: the table
    // on its way up (W0 9n | par 3 | gf, ints packed by two), then the results on their way down (values 2n | entry objectives S)
    const size_t o_parts = (size_t)2 * n, o_scal = o_parts + REDUCE_PARTS, o_entry = o_scal + 2;
    gp.d_gc_f.need(n); gp.d_gc_W0.need((size_t)9 * n); gp.d_gc_w.need(n); gp.d_gc_par.need(1); gp.d_gc_out.need(o_entry + S);
    HIPCHECK(hipStreamSynchronize(s));       // (the pinned staging buffer is written below)
    gp.gc_stage.need(std::max((size_t)9 * n + 3 + ((size_t)n + 1) / 2, (size_t)2 * n + S));
    static_assert(sizeof(GncPar) == 24, "GncPar travels as three 8-byte words");
    double *stg = gp.gc_stage.p;
    int *si = (int *)(stg + (size_t)9 * n + 3);
    for (int i = 0; i < n; i++) {
        const int p = gp.g2p[cand[i]];
        si[i] = p;
        memcpy(stg + (size_t)9 * i, gp.h_W.p + (size_t)9 * p, 72);
    }
    GncPar par{ 1.0, o->c, o->loss, 0 };
    memcpy(stg + (size_t)9 * n, &par, sizeof par);
    HIPCHECK(hipMemcpyAsync(gp.d_gc_W0.p, stg, (size_t)72 * n, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(gp.d_gc_par.p, stg + (size_t)9 * n, sizeof par, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(gp.d_gc_f.p, si, (size_t)4 * n, hipMemcpyHostToDevice, s));
    // from here to the return the candidates carry the surrogate; a captured LM iteration of this run serves no other (gc_gen)
    struct Active {
        GraphPack &gp;
        Active(GraphPack &p, int n) : gp(p) { gp.gc_n = n; gp.gc_gen++; }
        ~Active() { gp.gc_n = 0; gp.gc_gen++; }
    } active(gp, n);
    lm_enter(c, gp, s, &o->lm);
    double *out = gp.d_gc_out.p;
    const int *fa = gp.d_fa.p, *fb = gp.d_fb.p; const double *Z = gp.d_z.p, *st = gp.d_state.p;
    // the start: s_max over the candidates at the incoming states
    launch_gnc(s, gp, k_gnc_probe, 0, fa, fb, Z, st, out);
    enqueue_reduce(REDUCE_MAX, s, n, out, out + o_parts, out + o_scal);
    HIPCHECK(hipMemcpyAsync(stg, out + o_scal, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const double s_max = stg[0];
    double mu = tls ? (2.0 * s_max > cc ? cc / (2.0 * s_max - cc) : (double)INFINITY) : std::max(1.0, 2.0 * s_max / cc);
    const double mu0 = mu;
    LmScalars &h = *c.h_lm.p;
    std::vector<double> rows;
    int status = 0, stages = 0, iterations = 0, accepted = 0, stalled = 0;
    while (status == 0) {
        hipLaunchKernelGGL(k_gnc_set_mu, dim3(1), dim3(64), 0, s, gp.d_gc_par.p, mu);
        lm_enqueue_start(c, gp, s, &o->lm, false);
        HIPCHECK(hipMemcpyAsync(out + o_entry + stages, &c.d_lm.p->F, 8, hipMemcpyDeviceToDevice, s));      // (F on entry under this mu: read at the end)
        lm_iterate(c, gp, s, &o->lm);
        rows.insert(rows.end(), { mu, 0.0, h.F, (double)h.iterations });
        stages++; iterations += h.iterations; accepted += h.accepted; stalled += h.status == LM_STALLED;
        bool done = mu == 1.0;
        if (tls) {        // every weight exactly 0 or 1 at the stage's final x?
            launch_gnc(s, gp, k_gnc_probe, 1, fa, fb, Z, st, out);
            enqueue_reduce(REDUCE_MAX, s, n, out, out + o_parts, out + o_scal + 1);
            HIPCHECK(hipMemcpyAsync(stg, out + o_scal + 1, 8, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
            done = stg[0] == 0.0;
        }
        if (done) status = 1;
        else if (stages >= S) status = 2;
        else mu = tls ? mu * o->mu_step : std::max(1.0, mu / o->mu_step);
    }
    // results: w_mu(s) and the inlier test at the returned states, the plain W back in the candidates' slots (before the plain chi^2)
    launch_gnc(s, gp, k_gnc_final, fa, fb, Z, st, gp.d_W.p, out);
    HIPCHECK(hipMemcpyAsync(stg, out, (size_t)16 * n, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(stg + (size_t)2 * n, out + o_entry, (size_t)8 * stages, hipMemcpyDeviceToHost, s));
    const double F_final = h.F;
    const double chi2 = lm_write_back(c, gp, s, g);       // (synchronises the stream)
    int inl = 0;
    for (int i = 0; i < n; i++) inl += stg[n + i] != 0.0;
    if (weights) memcpy(weights, stg, (size_t)8 * n);
    for (int k = 0; k < stages; k++) rows[(size_t)4 * k + 1] = stg[(size_t)2 * n + k];
    if (stage_trace) memcpy(stage_trace, rows.data(), rows.size() * 8);
    report->status = status; report->stages = stages; report->iterations = iterations; report->accepted = accepted; report->stages_stalled = stalled;
    report->n_inliers = inl; report->mu_initial = mu0; report->mu_final = mu; report->s_max = s_max;
    report->F_final = F_final; report->chi2_final = chi2;
    return 0;
}

int optimize_gnc(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_gnc_opts_t *opts, int n, const int *cand,
                 aprilsam_amd_gnc_report_t *report, double *weights, double *stage_trace) {
    const char *who = "aprilsam_amd_optimize_gnc";
    char msg[256];
    if (!g || !param || !opts || !report || !cand) { snprintf(msg, sizeof msg, "%s: null argument", who); return gate_refuse(ERR_BAD_GRAPH, msg); }
    if (const char *why = gnc_bad_options(opts)) { snprintf(msg, sizeof msg, "%s: bad options: %s", who, why); return gate_refuse(ERR_BAD_GRAPH, msg); }
    if (zsize(g->nodes) == 0 || zsize(g->factors) == 0) { snprintf(msg, sizeof msg, "%s: empty graph", who); return gate_refuse(-1, msg); }
    if (n <= 0) { snprintf(msg, sizeof msg, "%s: n = %d candidates", who, n); return gate_refuse(ERR_BAD_GRAPH, msg); }
    {   // the candidates: distinct plain xyt / xytpos factors of this library with a symmetric positive definite W
        const int Fg = zsize(g->factors);
        april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
        std::vector<char> seen((size_t)Fg, 0);
        for (int i = 0; i < n; i++) {
            const int k = cand[i];
            if (k < 0 || k >= Fg) { snprintf(msg, sizeof msg, "%s: candidate %d: factor index %d out of range (%d factors)", who, i, k, Fg); return gate_refuse(ERR_BAD_GRAPH, msg); }
            if (seen[k]) { snprintf(msg, sizeof msg, "%s: candidate %d: factor %d is listed twice", who, i, k); return gate_refuse(ERR_BAD_GRAPH, msg); }
            seen[k] = 1;
        }
        for (int i = 0; i < n; i++) {
            const april_graph_factor_t *f = fs[cand[i]];
            int kind = 0; double rc = 0;
            const char *why = nullptr;
            if (is_native_max(f)) why = "is a max factor";       // (before anything reads u.common: u.max aliases it)
            else if (!plain_common_factor(f)) why = "is not an xyt / xytpos factor of this library";
            else if (robust_of(f, &kind, &rc)) why = "already carries a robust loss";
            else if (!robust_spd(f->u.common.W->data)) why = "has a W that is not symmetric positive definite";
            if (why) { snprintf(msg, sizeof msg, "%s: candidate %d (factor %d) %s", who, i, cand[i], why); return gate_refuse(ERR_UNSUPPORTED, msg); }
        }
    }
    return guarded_rc(param, g, [&] { return optimize_gnc_impl(g, param, opts, n, cand, report, weights, stage_trace); });
}
