// solver_chordal.inc.h -- part of solver.hip.cpp (ONE translation unit), included from there, inside namespace asam.  Contents: the driver of
// aprilsam_amd_initialize_chordal, chordal initialisation of the poses (kernels in chordal.hip.h).
//
// Set-up is resident_begin_impl's (pack, plan, upload; a new plan is made without the coordinate hint).  Each stage is the numeric phase of a batch step with its contribution slots filled
// by k_chordal_rot / k_chordal_trans instead of the linearisation (enqueue_numeric's fill), damping 0, and its state update pointed at a
// scratch buffer: the solution itself is what the back substitution leaves in d_dx (node order).  The call runs once or twice in a graph's
// lifetime, so nothing is captured.  The end copies the states back as LM does and drops the retained factor.

void chordal_opts_init(aprilsam_amd_chordal_opts_t *o) {
    if (!o) return;
    o->stages = 3;
}

// the slots of stage `stage` (1 / 2): every packed factor from its own z / W, then the robust factors again from their unweighted W, then
// the max factors from the component chosen for them (later launches overwrite earlier ones: one stream)
static void chordal_enqueue_fill(Context &c, GraphPack &gp, hipStream_t s, int stage, const double *theta) {
    const int F = gp.F, R = gp.n_robust(), M = gp.n_max();
    auto launch = [&](int n, ChordalSrc src, bool first) {
        int *bad = first ? c.d_bad.p : nullptr, *epoch = first ? c.d_epoch.p : nullptr;
        if (stage == 1)
            hipLaunchKernelGGL(k_chordal_rot, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, n, src, gp.d_fa.p, gp.d_fb.p, c.d_swap.p, c.dp.slot_blk, c.dp.slot_rhs,
                               c.d_H.p, bad, epoch);
        else
            hipLaunchKernelGGL(k_chordal_trans, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, n, src, gp.d_fa.p, gp.d_fb.p, theta, c.d_swap.p, c.dp.slot_blk,
                               c.dp.slot_rhs, c.d_H.p, bad, epoch);
    };
    launch(F, ChordalSrc{ nullptr, nullptr, nullptr, gp.d_z.p, gp.d_W.p }, true);
    if (R > 0) launch(R, ChordalSrc{ gp.d_rb_f.p, gp.d_rb_f.p, nullptr, gp.d_z.p, gp.d_rb_W0.p }, false);
    if (M > 0) launch(M, ChordalSrc{ gp.d_mx_f.p, c.d_ch_sel.p, c.d_ch_sel.p, gp.d_mx_z.p, gp.d_mx_W.p }, false);
}

// 1 / 2: the first stage whose system is singular by its structure -- a set of poses, connected by the stage's contributing xyt factors,
// that none of its contributing priors reaches (a pose without any contributing factor is such a set) -- or 0.  With positive weights this
// is exactly when the stage's matrix is not positive definite; the pivots cannot be trusted to say so: rounding leaves the last pivot of
// such a system tiny but positive as often as not, and stage 1 without a heading prior then "solves" to u = 0 everywhere.
static int chordal_unanchored_stage(const GraphPack &gp, const std::vector<int> &sel, int stages) {
    const int N = gp.N, F = gp.F;
    std::vector<const double *> Wp(F);
    for (int f = 0; f < F; f++) Wp[f] = gp.h_W.p + (size_t)9 * f;
    for (int q = 0; q < gp.n_robust(); q++) Wp[gp.rb_f[q]] = gp.rb_W0.data() + (size_t)9 * q;
    for (int m = 0; m < gp.n_max(); m++) Wp[gp.mx_f[m]] = gp.mx_W.data() + (size_t)9 * sel[m];
    std::vector<int> root(N);
    std::vector<char> anchored(N);
    auto find = [&](int i) { while (root[i] != i) { root[i] = root[root[i]]; i = root[i]; } return i; };
    for (int stage = 1; stage <= (stages == 3 ? 2 : 1); stage++) {
        for (int i = 0; i < N; i++) { root[i] = i; anchored[i] = 0; }
        for (int f = 0; f < F; f++) {
            const int a = gp.h_fa.p[f], b = gp.h_fb.p[f];
            const double *W = Wp[f];
            if (a < 0 || !(stage == 1 ? W[8] > 0 : (W[0] > 0 && W[0] * W[4] - W[1] * W[1] > 0))) continue;
            if (b < 0) { anchored[find(a)] = 1; continue; }
            const int ra = find(a), rb = find(b);
            if (ra != rb) { root[rb] = ra; anchored[ra] |= anchored[rb]; }
        }
        for (int i = 0; i < N; i++) if (!anchored[find(i)]) return stage;
    }
    return 0;
}

// one stage: fill, assemble + factor + back-substitute; true when every pivot was positive (the solution is in d_dx)
static bool chordal_run_stage(Context &c, GraphPack &gp, hipStream_t s, int stage, double *scratch, const double *theta) {
    rewind_epoch(c, s, 1);
    const std::function<void()> fill = [&] { chordal_enqueue_fill(c, gp, s, stage, theta); };
    NumericArgs a; a.st_dest = scratch; a.fill = &fill;
    enqueue_numeric(c, gp, s, a);
    HIPCHECK(hipMemcpyAsync(c.h_bad.p, c.d_bad.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const bool not_spd = check_bad(c);             // (a dependency time-out fails the call: ERR_DEP_TIMEOUT)
    check_guard(c, s);
    return !not_spd;
}

static int initialize_chordal_impl(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_chordal_opts_t *o,
                                   aprilsam_amd_chordal_report_t *report, double *rot_out, double *raw_out) {
    const char *who = "aprilsam_amd_initialize_chordal";
    char msg[256];
    ensure_device();
    {   // refusals before anything is uploaded: the param keeps whatever it had
        SlotLock lk(param, g);
        if (g_shard.find(param) != g_shard.end()) { snprintf(msg, sizeof msg, "%s: sharded params are not supported", who); return gate_refuse(ERR_UNSUPPORTED, msg); }
        if (int rc = refuse_fixed(who, g)) return rc;          // (fixed nodes, DESIGN.md section 20: the two linear stages know no mask yet)
        GraphPack &gp = pack_for(g);
        pack_factors(gp, g);
        if (!gp.host_idx.empty()) { snprintf(msg, sizeof msg, "%s: the graph holds host-evaluated factors (foreign types): use april_graph_cholesky", who); return gate_refuse(-4, msg); }
        if (gp.n_asym > 0) { snprintf(msg, sizeof msg, "%s: a factor has an asymmetric information matrix", who); return gate_refuse(ERR_UNSUPPORTED, msg); }
        if (gp.n_polar() > 0) { snprintf(msg, sizeof msg, "%s: the graph holds polar factors, which carry no relative heading (DESIGN.md section 19)", who); return gate_refuse(ERR_UNSUPPORTED, msg); }
        if (gp.n_gaussian() > 0) { snprintf(msg, sizeof msg, "%s: the graph holds dense Gaussian factors, which the two linear stages do not know (DESIGN.md section 24)", who); return gate_refuse(ERR_UNSUPPORTED, msg); }
    }
    SlotLock lk(param, g);
    Context &c = ctx_for(param);
    GraphPack &gp = pack_for(g);
    hipStream_t s = gp.stream;
    // pack, plan, upload as resident_begin does -- except that a plan made here takes no hint from the nodes' coordinates: the call reads
    // no state, and two graphs that differ in their states alone get the same elimination order, hence the same bits
    pack_states(gp, g, false);
    orient_asymmetric(c, gp);
    const bool reused = prepare_plan(c, gp, g, true, false);
    flush_orientation(c, s);
    upload_factors(gp);
    c.st.n_nodes = gp.N; c.st.n_factors = gp.F; c.st.symbolic_reused = reused; c.st.not_spd = 0; c.st.error_code = 0;
    const int N = gp.N, F = gp.F, T = std::max(F, 2 * N), M = gp.n_max();
    set_small_attr();
    gp.mirror_sync = false; gp.lp_last_valid = false;
    c.d_ch.need((size_t)4 * N + 4); c.h_ch.need(4);
    c.d_lm_terms.need((size_t)T + REDUCE_PARTS);
    double *scratch = c.d_ch.p, *theta = scratch + (size_t)3 * N, *scal = theta + N;      // scal: F_initial, F_final, degenerate poses, min |u|^2
    double *terms = c.d_lm_terms.p, *parts = terms + T;
    std::vector<int> sel(M);
    for (int m = 0; m < M; m++) {       // a max factor enters as the component with the largest log weight, lowest index on a tie
        int best = gp.mx_k[m];
        for (int k = gp.mx_k[m] + 1; k < gp.mx_k[m + 1]; k++) if (gp.mx_logw[k] > gp.mx_logw[best]) best = k;
        sel[m] = best;
    }
    if (M > 0) { c.d_ch_sel.need(M); HIPCHECK(hipMemcpy(c.d_ch_sel.p, sel.data(), (size_t)4 * M, hipMemcpyHostToDevice)); }
    const int unanchored = chordal_unanchored_stage(gp, sel, o->stages);
    lm_enqueue_cost(c, gp, s, gp.d_state.p, scal);
    HIPCHECK(hipMemsetAsync(scal + 1, 0, 24, s));

    auto read_scalars = [&]() {
        HIPCHECK(hipMemcpyAsync(c.h_ch.p, scal, 32, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    };
    auto not_spd = [&](int stage) {          // the one refusal that writes the report; the graph's states were never written
        read_scalars();
        report->status = ERR_NOT_SPD; report->n_degenerate = 0; report->not_spd_stage = stage; report->min_norm = 0;
        report->F_initial = c.h_ch.p[0]; report->F_final = c.h_ch.p[0];
        snprintf(msg, sizeof msg, "%s: the system of stage %d is not positive definite (%s)", who, stage,
                 stage == 1 ? "no heading prior, or a part of the graph that none reaches" : "no position prior, or a part of the graph that none reaches");
        return gate_refuse(ERR_NOT_SPD, msg);
    };
    if (unanchored) return not_spd(unanchored);      // (before anything of the param is overwritten: its retained factor stays)

    // damping 0 for both stages; d_lambda no longer holds the param's value: whatever runs next on this param must rewrite it
    c.lambda_N = -1; c.lambda_val = -1;
    set_lambda(c, gp, 0.0);
    c.lambda_N = -1; c.lambda_val = -1;
    c.have_fact = false; c.fact_kind = FACT_NONE;          // (the stages factorise over the retained factor)
    HIPCHECK(hipMemcpyAsync(gp.d_lp.p, gp.d_state.p, (size_t)24 * N, hipMemcpyDeviceToDevice, s));

    // stage 1: headings
    if (!chordal_run_stage(c, gp, s, 1, scratch, nullptr)) return not_spd(1);
    std::vector<double> raw;
    if (rot_out || raw_out) { raw.resize((size_t)6 * N); HIPCHECK(hipMemcpyAsync(raw.data(), gp.d_dx.p, (size_t)24 * N, hipMemcpyDeviceToHost, s)); }
    hipLaunchKernelGGL(k_chordal_heading, dim3((N + TPB - 1) / TPB), dim3(TPB), 0, s, N, (const double *)gp.d_dx.p, (const double *)gp.d_state.p, theta, terms, terms + N);
    enqueue_reduce(REDUCE_SUM, s, N, terms + N, parts, scal + 2);
    enqueue_reduce(REDUCE_MIN, s, N, terms, parts, scal + 3);
    HIPCHECK(hipGetLastError());

    // stage 2: positions with the headings held fixed
    const bool both = o->stages == 3;
    if (both && !chordal_run_stage(c, gp, s, 2, scratch, theta)) return not_spd(2);
    if (both && raw_out) HIPCHECK(hipMemcpyAsync(raw.data() + (size_t)3 * N, gp.d_dx.p, (size_t)24 * N, hipMemcpyDeviceToHost, s));
    hipLaunchKernelGGL(k_chordal_commit, dim3((N + TPB - 1) / TPB), dim3(TPB), 0, s, N, both ? (const double *)gp.d_dx.p : (const double *)nullptr, (const double *)theta,
                       gp.d_state.p, gp.d_lp.p);
    lm_enqueue_cost(c, gp, s, gp.d_state.p, scal + 1);
    HIPCHECK(hipGetLastError());

    // results: state = l_point = the initial guess; delta_X stays
    HIPCHECK(hipMemcpyAsync(gp.h_state.p, gp.d_state.p, (size_t)24 * N, hipMemcpyDeviceToHost, s));
    read_scalars();
    memcpy(gp.h_lp.p, gp.h_state.p, (size_t)24 * N);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < N; i++) {
        memcpy(ns[i]->state, gp.h_state.p + (size_t)3 * i, 24);
        memcpy(ns[i]->l_point, gp.h_state.p + (size_t)3 * i, 24);
    }
    if (rot_out) for (int i = 0; i < N; i++) { rot_out[2 * i] = raw[(size_t)3 * i]; rot_out[2 * i + 1] = raw[(size_t)3 * i + 1]; }
    if (raw_out) memcpy(raw_out, raw.data(), (size_t)(both ? 48 : 24) * N);
    report->status = 0; report->n_degenerate = (int)c.h_ch.p[2]; report->not_spd_stage = 0; report->min_norm = std::sqrt(c.h_ch.p[3]);
    report->F_initial = c.h_ch.p[0]; report->F_final = c.h_ch.p[1];
    return 0;
}

// raw_out (debug, tests): NULL or 6 N doubles -- the stage-1 solution then the stage-2 solution, node order, padding included
int initialize_chordal(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_chordal_opts_t *opts, aprilsam_amd_chordal_report_t *report,
                       double *rot_out, double *raw_out) {
    const char *who = "aprilsam_amd_initialize_chordal";
    char msg[256];
    if (!g || !param || !opts || !report) { snprintf(msg, sizeof msg, "%s: null argument", who); return gate_refuse(ERR_BAD_GRAPH, msg); }
    if (opts->stages != 1 && opts->stages != 3) { snprintf(msg, sizeof msg, "%s: bad options: stages must be 3 (both) or 1 (headings only)", who); return gate_refuse(ERR_BAD_GRAPH, msg); }
    if (zsize(g->nodes) == 0 || zsize(g->factors) == 0) { snprintf(msg, sizeof msg, "%s: empty graph", who); return gate_refuse(-1, msg); }
    return guarded_rc(param, g, [&] { return initialize_chordal_impl(g, param, opts, report, rot_out, raw_out); });
}
