// solver_marginals.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: aprilsam_amd_marginals / aprilsam_amd_marginals_joint: marginal covariances of the system the last solver call
// factorised, by selected inversion of the retained factor (selinv.hip.h), and the extraction of the requested blocks.
// Admission, refusals, the guard and the structure the factor lives in: solver_query.inc.h (RetainedQuery, FactorView).
// ------------------------------------------------------------------------------------------------------
// The selected inversion's work entries for the current view, level by level (root first), and its scratch.  SelFront::scr is written
// on the VIEW's own fronts before they are uploaded: only the selinv kernels read it, and it depends on the view alone.
static void build_sel_tables(Context &c, hipStream_t s) {
    FactorView &V = factor_view(c);
    std::vector<SelFront> &fr = V.fr;
    const int nLev = (int)V.lev.size();
    std::vector<int4> ent;
    c.sel_tab_gen = -1;
    c.sel_levels.assign(nLev, SelLevel());
    long long scr_max = 16;
    for (int l = 0; l < nLev; l++) {                        // root first
        SelLevel &L = c.sel_levels[l];
        const std::vector<int> &fl = V.lev[l];
        long long scr = 0;
        for (int t : fl) { fr[t].scr = scr; scr += (long long)sel_round16(fr[t].s) * (sel_round16(fr[t].s) + sel_round16(fr[t].u)); }
        scr_max = std::max(scr_max, scr);
        // (the tile loops below walk each front's tiles in a fixed order: the tables, not the hardware, decide who writes what)
        L.gat = span_of(ent, [&] {
            for (int t : fl) if (fr[t].parent >= 0 && fr[t].u > 0) {
                const long long nel = (long long)fr[t].u * fr[t].u;
                for (long long ch = 0; ch * SEL_GATHER_PER_WG < nel; ch++) ent.push_back(int4{ t, (int)ch, 0, 0 });
            }
        });
        L.diag = span_of(ent, [&] { for (int t : fl) for (int b = 0; b * SEL_T < fr[t].s; b++) ent.push_back(int4{ t, b, 0, 0 }); });
        L.tri = span_of(ent, [&] {                          // (the longest chains -- column block 0 of the widest fronts -- first)
            std::vector<int4> tri;
            for (int t : fl) for (int b = 0; (b + 1) * SEL_T < fr[t].s; b++) tri.push_back(int4{ t, b, 0, 0 });
            std::stable_sort(tri.begin(), tri.end(), [&](const int4 &a, const int4 &b) { return fr[a.x].s - SEL_T * a.y > fr[b.x].s - SEL_T * b.y; });
            ent.insert(ent.end(), tri.begin(), tri.end());
        });
        auto us_tiles = [&] { for (int t : fl) for (int j = 0; j * SEL_T < fr[t].s; j++) for (int i = 0; i * SEL_T < fr[t].u; i++) ent.push_back(int4{ t, i, j, 0 }); };
        L.x = span_of(ent, us_tiles);
        L.sus = span_of(ent, us_tiles);
        L.sss = span_of(ent, [&] { for (int t : fl) for (int j = 0; j * SEL_T < fr[t].s; j++) for (int i = j; i * SEL_T < fr[t].s; i++) ent.push_back(int4{ t, i, j, 0 }); });
    }
    if (ent.empty()) ent.push_back(int4{ 0, 0, 0, 0 });
    c.d_sel_fd.need(std::max<size_t>(1, fr.size())); c.d_sel_ent.need(ent.size());
    c.d_sel_scr.need((size_t)scr_max);
    view_pos(c, s);
    if (!fr.empty()) HIPCHECK(hipMemcpyAsync(c.d_sel_fd.p, fr.data(), fr.size() * sizeof(SelFront), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(c.d_sel_ent.p, ent.data(), ent.size() * sizeof(int4), hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));                      // (the host vector goes out of scope)
    c.sel_tab_gen = V.gen;
}

// Sigma on the pattern of L, root to leaves: per level gather Sig_UU, invert L_SS, X = L_US Linv, Sig_US, Sig_SS
static void enqueue_selinv(Context &c, hipStream_t s) {
    const SelFront *fr = c.d_sel_fd.p; const int4 *ent = c.d_sel_ent.p;
    const int *rel = c.d_i32.p;                             // (the block maps the factorisation read)
    double *sig = c.d_sigma.p, *scr = c.d_sel_scr.p; const double *pool = c.d_pool.p;
    for (const SelLevel &L : c.sel_levels) {
        if (L.gat.n) hipLaunchKernelGGL(k_selinv_gather, dim3(L.gat.n), dim3(TPB), 0, s, fr, rel, ent + L.gat.off, sig);
        launch_waves(k_selinv_diag, s, L.diag, 1, fr, ent, pool, scr);
        launch_waves(k_selinv_trinv, s, L.tri, 1, fr, ent, pool, scr);
        launch_waves(k_selinv_x, s, L.x, 1, fr, ent, pool, scr);
        launch_waves(k_selinv_sus, s, L.sus, 1, fr, ent, (const double *)scr, sig);
        launch_waves(k_selinv_sss, s, L.sss, 1, fr, ent, (const double *)scr, sig);
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
// been synchronised.  Every consumer that reads Sigma calls it: the marginals, the factor audit, aprilsam_amd_relative_covariances.
static void sel_ensure(Context &c, hipStream_t s) {
    if (c.sel_serial == c.fact_serial) return;
    c.sel_serial = -1;
    if (c.sel_tab_gen != factor_view(c).gen) build_sel_tables(c, s);      // (the view's validity rule decides: solver_query.inc.h)
    c.d_sigma.need((size_t)c.view.pool_end);
    enqueue_selinv(c, s);
    c.sel_runs++;
}

static int marginals_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, double *cov, bool joint) {
    // (both entry points answer under the first one's name; only the null node list of the joint call names its own)
    const char *who = "aprilsam_amd_marginals";
    if (!param || !cov) return refuse(ERR_BAD_GRAPH, who, "null param or output");
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    const int N = q.N();
    std::vector<int> all;
    if (!qa) {
        if (joint) return refuse(ERR_BAD_GRAPH, "aprilsam_amd_marginals_joint", "null node list");
        if (g && zsize(g->nodes) != N) return q.refuse(ERR_BAD_GRAPH, "the graph has nodes the last solver call did not factorise");
        all.resize((size_t)N);
        for (int i = 0; i < N; i++) all[i] = i;
        qa = all.data(); n = N;
    }
    if (n < 0 || (joint && !qb)) return q.refuse(ERR_BAD_GRAPH, "bad node list");
    for (int i = 0; i < n; i++)
        if (qa[i] < 0 || qa[i] >= N || (joint && (qb[i] < 0 || qb[i] >= N)))
            return q.refuse(ERR_BAD_GRAPH, "node id out of range of the factorised system (nodes added since the last solver call?)");
    if (n == 0) return 0;
    hipStream_t s = q.stream();
    sel_ensure(c, s);
    const int *pos = view_pos(c, s);
    const int per = joint ? 36 : 9;
    c.d_sel_q.need((size_t)2 * n);
    HIPCHECK(hipMemcpyAsync(c.d_sel_q.p, qa, (size_t)4 * n, hipMemcpyHostToDevice, s));
    if (joint) HIPCHECK(hipMemcpyAsync(c.d_sel_q.p + n, qb, (size_t)4 * n, hipMemcpyHostToDevice, s));
    c.h_cov.need((size_t)per * n);
    const long long nv = (long long)per * n;
    hipLaunchKernelGGL(k_marginal_extract, dim3((unsigned)((nv + TPB - 1) / TPB)), dim3(TPB), 0, s, n, (const int *)c.d_sel_q.p,
                       joint ? (const int *)c.d_sel_q.p + n : (const int *)nullptr, pos, pos + N,
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
int marginals(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, double *cov, bool joint) {
    return query_guard([&] { return marginals_impl(g, param, n, qa, qb, cov, joint); });
}
long long selinv_runs(const april_graph_cholesky_param_t *param) { return context_field(param, [](const Context &c) { return c.sel_runs; }); }
