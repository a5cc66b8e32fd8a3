// solver_treesolve.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: aprilsam_amd_solve / aprilsam_amd_marginals_cross / aprilsam_amd_relative_covariances: solves with the retained factor for
// right-hand sides the caller supplies, as two whole-tree passes (treesolve.hip.h), and what is read from the solve of an anchor pose's
// unit columns.  DESIGN.md section 18.
// Admission, refusals, the guard and the structure the factor lives in: solver_query.inc.h (RetainedQuery, FactorView).
// ------------------------------------------------------------------------------------------------------
// The tables of the two passes for the current view, kept against its generation: the fronts' rows in the work buffer, the children of
// every parent block row (CSR, ascending front id: the order k_ts_assemble sums in), position -> node, and the work entries level by
// level.  None of them depends on the number of columns: PsFront::buf holds a front's first row in the work buffer, the kernels take
// the column count as an argument.  Returns pos | pos_front on the device (view_pos).
static const int *ts_tables(Context &c, hipStream_t s) {
    TreeState &T = c.ts;
    const FactorView &S = factor_view(c);
    if (T.gen == S.gen) return view_pos(c, s);
    T.gen = -1;
    const std::vector<SelFront> &fr = S.fr;
    const int nFr = (int)fr.size(), N = S.N;
    T.wrow.assign((size_t)nFr + 1, 0);
    long long rows = 0;
    int rel_end = 0;
    for (int t = 0; t < nFr; t++) {
        T.wrow[t] = (int)rows;
        rows += fr[t].s + fr[t].u;
        if (rows > 0x7fffffffll / 2) fail(ERR_UNSUPPORTED, "aprilsam_amd_solve: the fronts hold more than 2^30 rows");
        if (fr[t].parent >= 0 && fr[t].u > 0) rel_end = std::max(rel_end, fr[t].rel_begin + fr[t].u / 3);
    }
    T.wrow[nFr] = (int)rows;
    T.rows = rows;
    // the block maps the factorisation read (device arena), for the children lists
    std::vector<int> rel((size_t)std::max(rel_end, 1));
    if (rel_end > 0) {
        HIPCHECK(hipMemcpyAsync(rel.data(), c.d_i32.p, (size_t)4 * rel_end, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    const int nB = (int)(rows / 3);
    std::vector<int> cptr((size_t)nB + 1, 0);
    for (int t = 0; t < nFr; t++) {
        const SelFront &F = fr[t];
        if (F.parent < 0) continue;
        const SelFront &P = fr[F.parent];
        const int nbp = (P.s + P.u) / 3;
        for (int a = 0; a < F.u / 3; a++) {
            const int r = rel[(size_t)F.rel_begin + a];
            if (r < 0 || r >= nbp) fail(ERR_INTERNAL, "aprilsam_amd_solve: front %d: struct row %d maps to row %d of its parent's %d", t, a, r, nbp);
            cptr[(size_t)T.wrow[F.parent] / 3 + r + 1]++;
        }
    }
    for (int b = 0; b < nB; b++) cptr[b + 1] += cptr[b];
    std::vector<TsKid> cent((size_t)std::max(cptr[nB], 1));
    {
        std::vector<int> fill(cptr.begin(), cptr.end() - 1);
        for (int t = 0; t < nFr; t++) {                     // (ascending t: every list ends up in ascending child id)
            const SelFront &F = fr[t];
            if (F.parent < 0) continue;
            for (int a = 0; a < F.u / 3; a++)
                cent[(size_t)fill[(size_t)T.wrow[F.parent] / 3 + rel[(size_t)F.rel_begin + a]]++] = TsKid{ T.wrow[t], F.s + F.u, F.s + 3 * a, 0 };
        }
    }
    std::vector<int> npos((size_t)std::max(N, 1), 0);
    for (int i = 0; i < N; i++) {
        const int p = S.i32[i];
        if (p < 0 || p >= N) fail(ERR_INTERNAL, "aprilsam_amd_solve: node %d has position %d of %d", i, p, N);
        npos[p] = i;
        const SelFront &F = fr[S.i32[N + p]];
        if (p < F.first || 3 * (p - F.first) + 3 > F.s) fail(ERR_INTERNAL, "aprilsam_amd_solve: node %d is not among its front's own rows", i);
    }
    // work entries, level by level (root first)
    const int nLev = (int)S.lev.size();
    std::vector<int2> ent;
    T.lev.assign((size_t)nLev, TsLevel());
    for (int l = 0; l < nLev; l++) {
        TsLevel &L = T.lev[l];
        const std::vector<int> &fl = S.lev[l];
        L.assemble = span_of(ent, [&] { for (int t : fl) for (int b = 0; b * TS_BAND < fr[t].s + fr[t].u; b++) ent.push_back(int2{ t, b }); });
        L.trsm = span_of(ent, [&] {                         // (the longest chains first)
            std::vector<int> o(fl);
            std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return fr[a].s > fr[b].s; });
            for (int t : o) ent.push_back(int2{ t, 0 });
        });
        L.gemm = span_of(ent, [&] { for (int t : fl) for (int i = 0; i * SEL_T < fr[t].u; i++) ent.push_back(int2{ t, i }); });
        L.gather = span_of(ent, [&] { for (int t : fl) if (fr[t].parent >= 0) for (int b = 0; b * TS_BAND < fr[t].u; b++) ent.push_back(int2{ t, b }); });
        L.gemmt = span_of(ent, [&] { for (int t : fl) if (fr[t].u > 0) for (int i = 0; i * SEL_T < fr[t].s; i++) ent.push_back(int2{ t, i }); });
    }
    if (ent.empty()) ent.push_back(int2{ 0, 0 });
    std::vector<PsFront> pf((size_t)std::max(nFr, 1));
    for (int t = 0; t < nFr; t++) pf[t] = ps_front(fr[t], T.wrow[t], 0, fr[t].parent, 0);      // (buf: the first row; the column count is the kernels' argument)
    T.d_fr.need(std::max<size_t>(1, (size_t)nFr)); T.d_ent.need(ent.size()); T.d_cptr.need(cptr.size()); T.d_cent.need(cent.size());
    T.d_npos.need(npos.size());
    const int *pos = view_pos(c, s);
    HIPCHECK(hipMemcpyAsync(T.d_fr.p, pf.data(), pf.size() * sizeof(PsFront), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(T.d_ent.p, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(T.d_cptr.p, cptr.data(), cptr.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(T.d_cent.p, cent.data(), cent.size() * sizeof(TsKid), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(T.d_npos.p, npos.data(), npos.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));                      // (the host vectors go out of scope)
    T.gen = S.gen;
    return pos;
}

// the columns of one chunk: how many keep the work buffer under 1 GB / mem_cap_mb (ps_budget), a multiple of 16 and at least 16; option
// solve_chunk_cols forces the width.  A buffer that does not fit under mem_cap_mb even so is refused by its allocation (ERR_OOM).
static int ts_chunk_cols(const TreeState &T, int ncol) {
    long long w = g_opt.solve_chunk_cols > 0 ? ((long long)g_opt.solve_chunk_cols + 15) / 16 * 16 : std::max(16ll, ps_budget() / std::max(T.rows, 1ll) / 16 * 16);
    w = std::min(w, 1ll << 16);                             // (the column tiles are the grid's y dimension)
    return (int)std::min<long long>(w, ncol);
}

// One chunk: the passes of `mode` over ncol columns; dB = the right-hand sides on the device, [ncol][3 N] in node order.  The result is
// left in the fronts' own rows of the work buffer (k_ts_store / k_cross_extract / k_relative_cov read it).
static void ts_passes(Context &c, hipStream_t s, int mode, int ncol, const double *dB) {
    TreeState &T = c.ts;
    const PsFront *fr = T.d_fr.p; const int2 *ent = T.d_ent.p;
    const double *pool = c.d_pool.p; double *buf = T.d_buf.p;
    const long long n3 = 3ll * c.view.N;
    const unsigned ct = (unsigned)((ncol + SEL_T - 1) / SEL_T);
    const int nLev = (int)T.lev.size();
    const bool fwd = mode != APRILSAM_AMD_SOLVE_BACKWARD, bwd = mode != APRILSAM_AMD_SOLVE_FORWARD;
    auto assemble = [&](const TsLevel &L, int kids) {
        if (L.assemble.n) hipLaunchKernelGGL(k_ts_assemble, dim3(L.assemble.n), dim3(256), 0, s, fr, ent + L.assemble.off, (const int *)T.d_cptr.p, (const TsKid *)T.d_cent.p,
                                             (const int *)T.d_npos.p, dB, n3, 1, kids, ncol, buf);
    };
    if (fwd)
        for (int l = nLev - 1; l >= 0; l--) {
            const TsLevel &L = T.lev[l];
            assemble(L, 1);
            launch_waves(k_ts_trsm, s, L.trsm, ct, fr, ent, pool, ncol, buf);
            launch_waves(k_ts_gemm, s, L.gemm, ct, fr, ent, pool, ncol, buf);
        }
    if (bwd)
        for (int l = 0; l < nLev; l++) {
            const TsLevel &L = T.lev[l];
            if (!fwd) assemble(L, 0);
            if (L.gather.n) hipLaunchKernelGGL(k_ts_gather, dim3(L.gather.n), dim3(256), 0, s, fr, (const int *)c.d_i32.p, ent + L.gather.off, ncol, buf);
            launch_waves(k_ts_gemmt, s, L.gemmt, ct, fr, ent, pool, ncol, buf);
            launch_waves(k_ts_trsmt, s, L.trsm, ct, fr, ent, pool, ncol, buf);
        }
    HIPCHECK(hipGetLastError());
}

// the work buffer for chunks of w columns
static void ts_buffer(Context &c, int w) {
    TreeState &T = c.ts;
    const long long d = std::max(T.rows * w, 1ll);
    T.d_buf.need((size_t)d);
    T.peak_bytes = std::max(T.peak_bytes, 8 * d);
}

static int solve_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int mode, int nrhs, const double *B, double *X) {
    const char *who = "aprilsam_amd_solve";
    if (!param || !B || !X || nrhs < 1 || mode < APRILSAM_AMD_SOLVE_FULL || mode > APRILSAM_AMD_SOLVE_BACKWARD)
        return refuse(ERR_BAD_GRAPH, who, "null argument, mode outside 0..2 or nrhs < 1");
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    hipStream_t s = q.stream();
    const int *pos = ts_tables(c, s);
    TreeState &T = c.ts;
    const int N = q.N();
    const size_t n3 = (size_t)3 * N;
    const int w = ts_chunk_cols(T, nrhs);
    ts_buffer(c, w);
    T.d_B.need(n3 * w); T.h_B.need(n3 * w); T.h_X.need(n3 * w);
    // (several chunks: the results are kept back until the last one has succeeded, so that a call that fails half-way writes nothing)
    std::vector<double> stage;
    if (nrhs > w) stage.resize(n3 * (size_t)nrhs);
    double *out = stage.empty() ? X : stage.data();
    for (int c0 = 0; c0 < nrhs; c0 += w) {
        const int nc = std::min(w, nrhs - c0);
        memcpy(T.h_B.p, B + n3 * c0, 8 * n3 * nc);
        HIPCHECK(hipMemcpyAsync(T.d_B.p, T.h_B.p, 8 * n3 * nc, hipMemcpyHostToDevice, s));
        ts_passes(c, s, mode, nc, T.d_B.p);
        const long long nv = (long long)n3 * nc;
        hipLaunchKernelGGL(k_ts_store, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, (const PsFront *)T.d_fr.p,
                           pos, pos + N, (const double *)T.d_buf.p, N, nc, T.h_X.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
        memcpy(out + n3 * c0, T.h_X.p, 8 * n3 * nc);
    }
    if (!stage.empty()) memcpy(X, stage.data(), 8 * n3 * (size_t)nrhs);
    return 0;
}

// what marginals_cross / relative_covariances share: the admission of a fresh session and the checks, the node list on the device (null: all
// nodes) and the FULL solve of the anchor's three unit columns, left in the work buffer.  0 with n and pos | pos_front on the device, or the code.
static int ts_anchor(RetainedQuery &q, int anchor, int &n, const int *nodes, bool need_graph, const int *&pos) {
    // fixed nodes: not taken yet, neither in the graph nor in the factor at hand
    if (int rc = refuse_fixed(q.who, q.g)) return rc;
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    if (!c.fact_fixed.empty())
        return q.refuse(ERR_UNSUPPORTED, "the retained factor was made with node %d fixed; this entry point does not take fixed nodes yet (DESIGN.md section 20)", c.fact_fixed[0]);
    const int N = q.N(), Ng = need_graph ? zsize(q.g->nodes) : N;
    bool ok = anchor >= 0 && anchor < N && anchor < Ng && (nodes || N <= Ng) && (!nodes || n >= 0);
    if (!nodes) n = N;
    for (int i = 0; ok && nodes && i < n; i++) ok = nodes[i] >= 0 && nodes[i] < N && nodes[i] < Ng;
    if (!ok) return q.refuse(ERR_BAD_GRAPH, "anchor or node id out of range of the factorised system (nodes added since the last solver call?), or a negative count");
    if (n == 0) return 0;
    hipStream_t s = q.stream();
    pos = ts_tables(c, s);
    TreeState &T = c.ts;
    const size_t n3 = (size_t)3 * N;
    ts_buffer(c, 3);
    T.d_B.need(n3 * 3); T.h_X.need((size_t)9 * n);
    if (nodes) {
        T.d_nodes.need((size_t)n);
        HIPCHECK(hipMemcpyAsync(T.d_nodes.p, nodes, (size_t)4 * n, hipMemcpyHostToDevice, s));
    }
    HIPCHECK(hipMemsetAsync(T.d_B.p, 0, 8 * n3 * 3, s));
    std::vector<long long> at(3);
    for (int k = 0; k < 3; k++) at[k] = (long long)k * n3 + 3ll * anchor + k;
    c.ps.d_at.need(3);
    HIPCHECK(hipMemcpyAsync(c.ps.d_at.p, at.data(), 24, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));                      // (at goes out of scope; nodes is the caller's)
    hipLaunchKernelGGL(k_path_init, dim3(1), dim3(256), 0, s, 3, (const long long *)c.ps.d_at.p, T.d_B.p);
    ts_passes(c, s, APRILSAM_AMD_SOLVE_FULL, 3, T.d_B.p);
    return 0;
}

static int cross_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov) {
    const char *who = "aprilsam_amd_marginals_cross";
    if (!param || !cov) return refuse(ERR_BAD_GRAPH, who, "null argument");
    RetainedQuery q(who, g, param);
    const int *pos = nullptr;
    if (int rc = ts_anchor(q, anchor, n, nodes, false, pos)) return rc;
    if (n == 0) return 0;
    TreeState &T = q.c().ts;
    hipStream_t s = q.stream();
    hipLaunchKernelGGL(k_cross_extract, dim3((unsigned)((9ll * n + 255) / 256)), dim3(256), 0, s, n, nodes ? (const int *)T.d_nodes.p : (const int *)nullptr,
                       (const PsFront *)T.d_fr.p, pos, pos + q.N(), (const double *)T.d_buf.p, T.h_X.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    memcpy(cov, T.h_X.p, (size_t)8 * 9 * n);
    return 0;
}

static int relative_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov) {
    const char *who = "aprilsam_amd_relative_covariances";
    if (!g || !param || !cov) return refuse(ERR_BAD_GRAPH, who, "null argument");
    RetainedQuery q(who, g, param);
    const int *pos = nullptr;
    if (int rc = ts_anchor(q, anchor, n, nodes, true, pos)) return rc;
    if (n == 0) return 0;
    Context &c = q.c(); TreeState &T = c.ts;
    hipStream_t s = q.stream();
    sel_ensure(c, s);                                       // Sig_aa, Sig_ii: the selected inversion's Sigma pool, as aprilsam_amd_marginals
    std::vector<double> st((size_t)3 * (n + 1));            // the anchor's state, then the listed nodes'
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int k = 0; k < 3; k++) st[k] = ns[anchor]->state[k];
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) st[3 * (i + 1) + k] = ns[nodes ? nodes[i] : i]->state[k];
    T.d_st.need(st.size());
    HIPCHECK(hipMemcpyAsync(T.d_st.p, st.data(), 8 * st.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_relative_cov, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, nodes ? (const int *)T.d_nodes.p : (const int *)nullptr, anchor,
                       (const double *)T.d_st.p, (const double *)T.d_st.p + 3, (const PsFront *)T.d_fr.p, pos,
                       pos + q.N(), (const double *)T.d_buf.p, (const double *)c.d_sigma.p, T.h_X.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    c.sel_serial = c.fact_serial;
    memcpy(cov, T.h_X.p, (size_t)8 * 9 * n);
    return 0;
}

int tree_solve(april_graph_t *g, april_graph_cholesky_param_t *param, int mode, int nrhs, const double *B, double *X) {
    return query_guard([&] { return solve_impl(g, param, mode, nrhs, B, X); });
}
int marginals_cross(april_graph_t *g, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov) {
    return query_guard([&] { return cross_impl(g, param, anchor, n, nodes, cov); });
}
int relative_covariances(april_graph_t *g, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov) {
    return query_guard([&] { return relative_impl(g, param, anchor, n, nodes, cov); });
}
long long tree_solve_bytes(const april_graph_cholesky_param_t *param) { return context_field(param, [](const Context &c) { return c.ts.peak_bytes; }); }
int factorised_nodes(const april_graph_cholesky_param_t *param) {
    return (int)context_field(param, [](const Context &c) { return no_retained_factor(c) ? -1 : retained_N(c); });
}
