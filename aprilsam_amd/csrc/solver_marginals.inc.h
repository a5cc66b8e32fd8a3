// solver_marginals.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: aprilsam_amd_marginals / aprilsam_amd_marginals_joint: marginal covariances of the system the last solver call
// factorised, by selected inversion of the retained factor (selinv.hip.h), and the extraction of the requested blocks.
// ------------------------------------------------------------------------------------------------------
// Launch tables of the selected inversion for the structure the factor lives in: the plan of the last batch step (FACT_PLAN), or that
// plan with the incremental path's appended tail fronts and regenerated descriptors (FACT_EXTENDED: Context::inc -- descriptors,
// current parents, block maps and tail rows in the device arena d_i32, exactly what the factorisation read).  Fronts are grouped by
// their depth below the root: a front's parent is always one group earlier.
// The fronts of that structure (SelFront, without the scratch offsets), their depth below the root, the end of the pool they occupy, the
// estimated flops of the inversion, and i32 = pos | pos_front (node -> elimination position, position -> owning front) of its N nodes.
// Shared with the path solves of solver_gating.inc.h.  Returns N.
static int sel_fronts(Context &c, std::vector<SelFront> &fr, std::vector<int> &depth, std::vector<int> &i32, long long &pool_end, double &flops) {
    const Plan &P = c.plan; const IncState &I = c.inc;
    const bool ext = c.fact_kind == FACT_EXTENDED;
    const int nF0 = P.nF, nFr = ext ? I.nF0 + (int)I.t_first.size() : P.nF, N = ext ? c.inc_N : P.N;
    if (ext && (I.nF0 != P.nF || I.Nb != P.N || (int)I.fd.size() < nFr || (int)I.parent.size() < nFr || (int)I.E.size() < nFr || (int)I.rel_begin.size() < nFr))
        fail(ERR_INTERNAL, "aprilsam_amd_marginals: incremental bookkeeping does not match the plan");
    flops = 0;
    fr.assign((size_t)nFr, SelFront());
    depth.assign((size_t)nFr, 0);
    pool_end = 1;
    for (int t = nFr - 1; t >= 0; t--) {
        SelFront &F = fr[t];
        int nsb, nub, nub_real, parent;
        if (ext) {
            const FrontDesc &D = I.fd[t];
            nsb = D.nsb; nub = D.nub; parent = I.parent[t];
            nub_real = (t < nF0 ? P.f_nub[t] : 0) + (int)I.E[t].size();          // (beyond these: the last tail front's phantom rows)
            if (t >= nF0 && nsb != I.t_cnt[t - nF0]) fail(ERR_INTERNAL, "aprilsam_amd_marginals: tail front %d: descriptor out of step", t);
            F.off = D.off; F.rows_begin = D.rows_begin; F.first = D.first; F.rel_begin = parent >= 0 ? I.rel_begin[t] : 0;
        } else {
            nsb = P.f_nsb[t]; nub = nub_real = P.f_nub[t]; parent = P.f_parent[t];
            F.off = P.f_off[t]; F.rows_begin = (int)(I.o_rows + P.f_rows_ptr[t]); F.first = P.f_first[t]; F.rel_begin = (int)(I.o_rel + P.f_rows_ptr[t]);
        }
        if (nub_real > nub || (parent >= 0 && parent <= t) || parent >= nFr)
            fail(ERR_INTERNAL, "aprilsam_amd_marginals: front %d: inconsistent structure (struct rows %d of %d, parent %d)", t, nub_real, nub, parent);
        F.s = 3 * nsb; F.u = 3 * nub_real; F.R = 3 * (nsb + nub + 1); F.parent = parent; F.nsb = nsb;
        depth[t] = parent < 0 ? 0 : depth[parent] + 1;
        pool_end = std::max(pool_end, F.off + (long long)F.R * 3 * (nsb + nub));
        flops += 2.0 * F.u * F.u * F.s + (double)F.u * F.s * F.s + (double)F.s * F.s * F.s / 3.0;
    }
    i32.assign((size_t)2 * N, 0);                           // pos | pos_front
    for (int i = 0; i < N; i++) i32[i] = i < P.N ? P.pos[i] : i;                 // (a tail pose's position is its id)
    for (int t = 0; t < nF0; t++) for (int q = P.f_first[t]; q < P.f_first[t] + P.f_nsb[t]; q++) i32[N + q] = t;
    for (int q = P.N; q < N; q++) i32[N + q] = I.tf_of[q - P.N];
    return N;
}

// the selected inversion's work entries, level by level (root first), and its scratch
static void build_sel_tables(Context &c, hipStream_t s) {
    std::vector<SelFront> fr; std::vector<int> depth, i32; long long pool_end;
    const int N = sel_fronts(c, fr, depth, i32, pool_end, c.sel_flops), nFr = (int)fr.size();
    const int nLev = nFr ? *std::max_element(depth.begin(), depth.end()) + 1 : 0;
    std::vector<std::vector<int>> lev((size_t)nLev);
    for (int t = 0; t < nFr; t++) lev[depth[t]].push_back(t);
    std::vector<int4> ent;
    c.sel_levels.assign(nLev, SelLevel());
    long long scr_max = 16;
    for (int l = 0; l < nLev; l++) {                        // root first
        SelLevel &L = c.sel_levels[l];
        const std::vector<int> &fl = lev[l];
        long long scr = 0;
        for (int t : fl) { fr[t].scr = scr; scr += (long long)sel_round16(fr[t].s) * (sel_round16(fr[t].s) + sel_round16(fr[t].u)); }
        scr_max = std::max(scr_max, scr);
        // (the tile loops below walk each front's tiles in a fixed order: the tables, not the hardware, decide who writes what)
        L.gat_off = (int)ent.size();
        for (int t : fl) if (fr[t].parent >= 0 && fr[t].u > 0) {
            const long long nel = (long long)fr[t].u * fr[t].u;
            for (long long ch = 0; ch * SEL_GATHER_PER_WG < nel; ch++) ent.push_back(int4{ t, (int)ch, 0, 0 });
        }
        L.n_gat = (int)ent.size() - L.gat_off;
        L.diag_off = (int)ent.size();
        for (int t : fl) for (int b = 0; b * SEL_T < fr[t].s; b++) ent.push_back(int4{ t, b, 0, 0 });
        L.n_diag = (int)ent.size() - L.diag_off;
        // (trinv: the longest chains -- column block 0 of the widest fronts -- first)
        L.tri_off = (int)ent.size();
        {
            std::vector<int4> tri;
            for (int t : fl) for (int b = 0; (b + 1) * SEL_T < fr[t].s; b++) tri.push_back(int4{ t, b, 0, 0 });
            std::stable_sort(tri.begin(), tri.end(), [&](const int4 &a, const int4 &b) { return fr[a.x].s - SEL_T * a.y > fr[b.x].s - SEL_T * b.y; });
            ent.insert(ent.end(), tri.begin(), tri.end());
        }
        L.n_tri = (int)ent.size() - L.tri_off;
        L.x_off = (int)ent.size();
        for (int t : fl) for (int j = 0; j * SEL_T < fr[t].s; j++) for (int i = 0; i * SEL_T < fr[t].u; i++) ent.push_back(int4{ t, i, j, 0 });
        L.n_x = (int)ent.size() - L.x_off;
        L.sus_off = (int)ent.size();
        for (int t : fl) for (int j = 0; j * SEL_T < fr[t].s; j++) for (int i = 0; i * SEL_T < fr[t].u; i++) ent.push_back(int4{ t, i, j, 0 });
        L.n_sus = (int)ent.size() - L.sus_off;
        L.sss_off = (int)ent.size();
        for (int t : fl) for (int j = 0; j * SEL_T < fr[t].s; j++) for (int i = j; i * SEL_T < fr[t].s; i++) ent.push_back(int4{ t, i, j, 0 });
        L.n_sss = (int)ent.size() - L.sss_off;
    }
    if (ent.empty()) ent.push_back(int4{ 0, 0, 0, 0 });
    c.sel_N = N; c.sel_pool = pool_end;
    c.d_sel_fd.need(std::max<size_t>(1, fr.size())); c.d_sel_i32.need(std::max<size_t>(1, i32.size())); c.d_sel_ent.need(ent.size());
    c.d_sel_scr.need((size_t)scr_max);
    if (!fr.empty()) HIPCHECK(hipMemcpyAsync(c.d_sel_fd.p, fr.data(), fr.size() * sizeof(SelFront), hipMemcpyHostToDevice, s));
    if (!i32.empty()) HIPCHECK(hipMemcpyAsync(c.d_sel_i32.p, i32.data(), i32.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(c.d_sel_ent.p, ent.data(), ent.size() * sizeof(int4), hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));                      // (the host vectors go out of scope)
    c.sel_tab_serial = c.fact_serial;
}

// Sigma on the pattern of L, root to leaves: per level gather Sig_UU, invert L_SS, X = L_US Linv, Sig_US, Sig_SS
static void enqueue_selinv(Context &c, hipStream_t s) {
    const SelFront *fr = c.d_sel_fd.p; const int4 *ent = c.d_sel_ent.p;
    const int *rel = c.d_i32.p;                             // (the block maps the factorisation read)
    double *sig = c.d_sigma.p, *scr = c.d_sel_scr.p; const double *pool = c.d_pool.p;
    auto waves = [](int n) { return dim3((unsigned)((n + 3) / 4)); };
    for (const SelLevel &L : c.sel_levels) {
        if (L.n_gat) hipLaunchKernelGGL(k_selinv_gather, dim3(L.n_gat), dim3(TPB), 0, s, fr, rel, ent + L.gat_off, sig);
        if (L.n_diag) hipLaunchKernelGGL(k_selinv_diag, waves(L.n_diag), dim3(TPB), 0, s, fr, ent + L.diag_off, L.n_diag, pool, scr);
        if (L.n_tri) hipLaunchKernelGGL(k_selinv_trinv, waves(L.n_tri), dim3(TPB), 0, s, fr, ent + L.tri_off, L.n_tri, pool, scr);
        if (L.n_x) hipLaunchKernelGGL(k_selinv_x, waves(L.n_x), dim3(TPB), 0, s, fr, ent + L.x_off, L.n_x, pool, scr);
        if (L.n_sus) hipLaunchKernelGGL(k_selinv_sus, waves(L.n_sus), dim3(TPB), 0, s, fr, ent + L.sus_off, L.n_sus, (const double *)scr, sig);
        if (L.n_sss) hipLaunchKernelGGL(k_selinv_sss, waves(L.n_sss), dim3(TPB), 0, s, fr, ent + L.sss_off, L.n_sss, (const double *)scr, sig);
    }
    HIPCHECK(hipGetLastError());
}

// what a successful solver call left in the front pool (Context::fact_kind), stamped with the step counter of its numeric phase: any
// later phase (a resident step, an incremental step, a failed call) moves the counter on and the stamp no longer matches
// (rewind_epoch forgets the factor when it starts the counter over).  fact_serial numbers the factorisations: Sigma and its tables are
// kept against it.
static void record_factor(Context &c, int kind, GraphPack &gp) {
    c.resident_open = false;                                // (a successful solver call: whatever loop was open before it is over)
    c.fact_kind = kind; c.fact_epoch = c.epoch_steps; c.fact_asym = gp.n_asym > 0 || c.wt_any; c.fact_serial++;
    c.fact_fixed = gp.fx_nodes;
    c.fact_pack = gp.serial; c.fact_upt = false;
    gp.lin_ctx = &c; gp.lin_serial = c.fact_serial; gp.lin_content = gp.content_version;      // (the pack holds THIS factorisation's linearisation)
}
// Fixed nodes: the consumers of the retained factor describe the system it was made from, identity blocks
// included.  A node fixed or freed since then makes that system another one: the factor is dropped, and the consumer answers as without.
static void drop_factor_if_toggled(Context &c, const april_graph_t *g) {
    if (!g || (c.fact_fixed.empty() && !fixed_ever())) return;
    std::vector<int> now;
    scan_fixed(g, now);
    if (now != c.fact_fixed) { c.have_fact = false; c.fact_kind = FACT_NONE; }
}
// per query i of n: bit 0 = qa[i] is among the fixed nodes of the retained factor, bit 1 = qb[i] (qb may be null); false when no bit is set
static bool fixed_query_mask(const Context &c, int n, const int *qa, const int *qb, std::vector<int> &mask) {
    if (c.fact_fixed.empty()) return false;
    bool any = false;
    mask.assign((size_t)n, 0);
    auto is = [&](int q) { return std::binary_search(c.fact_fixed.begin(), c.fact_fixed.end(), q); };
    for (int i = 0; i < n; i++) { mask[i] = (is(qa[i]) ? 1 : 0) | (qb && is(qb[i]) ? 2 : 0); any = any || mask[i]; }
    return any;
}

// Sigma of the retained factor on stream s, unless it is there already; the caller stamps c.sel_serial = c.fact_serial once the stream has
// been synchronised.  Shared with aprilsam_amd_relative_covariances (solver_treesolve.inc.h).
static void sel_ensure(Context &c, hipStream_t s) {
    if (c.sel_serial == c.fact_serial) return;
    c.sel_serial = -1;
    // (the plan's tables serve every factor of that plan; an extended structure changes with every incremental step)
    if (c.sel_tab_serial < 0 || c.fact_kind == FACT_EXTENDED || c.sel_tab_kind != FACT_PLAN) build_sel_tables(c, s);
    c.sel_tab_kind = c.fact_kind;
    c.d_sigma.need((size_t)c.sel_pool);
    enqueue_selinv(c, s);
    c.sel_runs++;
}

static int marginals_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, double *cov, bool joint) {
    auto refuse = [](int code, const char *msg) { set_last_error(code, msg); fprintf(stderr, "aprilsam_amd: ERROR %d: %s\n", code, msg); fflush(stderr); return code; };
    if (!param || !cov) return refuse(ERR_BAD_GRAPH, "aprilsam_amd_marginals: null param or output");
    ensure_device();
    SlotLock lk(param, g);
    if (g_shard.find(param) != g_shard.end()) return refuse(ERR_UNSUPPORTED, "aprilsam_amd_marginals: sharded params are not supported");
    auto it = g_ctx.find(param);
    if (it != g_ctx.end()) drop_factor_if_toggled(*it->second, g);
    if (it == g_ctx.end() || no_retained_factor(*it->second))
        return refuse(-1, "aprilsam_amd_marginals: no retained factor (no successful solver call since the param was created or last failed)");
    Context &c = *it->second;
    if (c.fact_asym) return refuse(ERR_UNSUPPORTED, "aprilsam_amd_marginals: the factorised graph holds factors with an asymmetric information matrix");
    const int N = c.fact_kind == FACT_EXTENDED ? c.inc_N : c.plan.N;
    std::vector<int> all;
    if (!qa) {
        if (joint) return refuse(ERR_BAD_GRAPH, "aprilsam_amd_marginals_joint: null node list");
        if (g && zsize(g->nodes) != N) return refuse(ERR_BAD_GRAPH, "aprilsam_amd_marginals: the graph has nodes the last solver call did not factorise");
        all.resize((size_t)N);
        for (int i = 0; i < N; i++) all[i] = i;
        qa = all.data(); n = N;
    }
    if (n < 0 || (joint && !qb)) return refuse(ERR_BAD_GRAPH, "aprilsam_amd_marginals: bad node list");
    for (int i = 0; i < n; i++)
        if (qa[i] < 0 || qa[i] >= N || (joint && (qb[i] < 0 || qb[i] >= N)))
            return refuse(ERR_BAD_GRAPH, "aprilsam_amd_marginals: node id out of range of the factorised system (nodes added since the last solver call?)");
    if (n == 0) return 0;
    hipStream_t s = take_stream(t_slot);
    struct Park { int slot; hipStream_t s; ~Park() { park_stream(slot, s); } } park{ t_slot, s };
    sel_ensure(c, s);
    const int per = joint ? 36 : 9;
    c.d_sel_q.need((size_t)2 * n);
    HIPCHECK(hipMemcpyAsync(c.d_sel_q.p, qa, (size_t)4 * n, hipMemcpyHostToDevice, s));
    if (joint) HIPCHECK(hipMemcpyAsync(c.d_sel_q.p + n, qb, (size_t)4 * n, hipMemcpyHostToDevice, s));
    c.h_cov.need((size_t)per * n);
    const long long nv = (long long)per * n;
    hipLaunchKernelGGL(k_marginal_extract, dim3((unsigned)((nv + TPB - 1) / TPB)), dim3(TPB), 0, s, n, (const int *)c.d_sel_q.p,
                       joint ? (const int *)c.d_sel_q.p + n : (const int *)nullptr, (const int *)c.d_sel_i32.p, (const int *)c.d_sel_i32.p + c.sel_N,
                       (const SelFront *)c.d_sel_fd.p, (const int *)c.d_i32.p, (const double *)c.d_sigma.p, c.h_cov.p);
    std::vector<int> fmask;
    if (fixed_query_mask(c, n, qa, joint ? qb : nullptr, fmask)) {      // fixed nodes: their rows and columns leave as exact zeros (k_fix_cov, on the pinned result)
        c.d_fx_mask.need((size_t)n);
        HIPCHECK(hipMemcpyAsync(c.d_fx_mask.p, fmask.data(), (size_t)4 * n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fix_cov, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, n, (const int *)c.d_fx_mask.p, per, c.h_cov.p, (double *)nullptr);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    c.sel_serial = c.fact_serial;
    memcpy(cov, c.h_cov.p, (size_t)8 * nv);
    if (!joint) return 0;
    int off = 0;
    for (int i = 0; i < n; i++) off += std::isnan(cov[(size_t)36 * i]) ? 1 : 0;
    return off;
}
// A failed marginals call only READS the param's plan and factor: unlike the solver entry points it records the error and leaves both
// in place (the next solver call is unaffected).
int marginals(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, double *cov, bool joint) {
    try { return marginals_impl(g, param, n, qa, qb, cov, joint); }
    catch (const SolverError &e) { set_last_error(e.code, e.msg); fprintf(stderr, "aprilsam_amd: ERROR %d: %s\n", e.code, e.msg.c_str()); fflush(stderr); (void)hipGetLastError(); return e.code; }
    catch (const std::bad_alloc &) { set_last_error(ERR_OOM, "host memory exhausted (std::bad_alloc)"); return ERR_OOM; }
    catch (const std::exception &e) { set_last_error(ERR_INTERNAL, e.what()); return ERR_INTERNAL; }
}
long long selinv_runs(const april_graph_cholesky_param_t *param) {
    SlotLock lk(param, nullptr);
    auto it = g_ctx.find(param);
    return it == g_ctx.end() ? -1 : it->second->sel_runs;
}
