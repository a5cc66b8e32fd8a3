// solver_audit.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: aprilsam_amd_factor_audit: per factor of the system the last solver call factorised, its share of the linear cost, its
// leverage, its leave-one-out distance and its checkability (audit.hip.h), from the selected inversion's Sigma pool
// (solver_marginals.inc.h) and the linearisation slots of the graph's pack.  DESIGN.md section 23.
// Admission, refusals and the guard: solver_query.inc.h (RetainedQuery).
// ------------------------------------------------------------------------------------------------------
// The second step of an admitted session, for the calls that read the contribution slots, d_lp and d_dx of the graph's pack as the
// param's last factorisation saw them (the factor audit; the marginal prior, solver_marginal_prior.inc.h): 0 with the pack and Fg, the
// number of graph factors wholly inside the factorised entries -- or the refusal's code (-1 / -12 / -13), recorded.  `what` names the
// caller's product in the messages ("the audit").
int RetainedQuery::linearisation(const char *what, GraphPack *&gpp, int &Fg) {
    Context &c = *cp;
    if (c.fact_kind == FACT_EXTENDED)
        return refuse(ERR_UNSUPPORTED, "the retained factor is an incremental step's extended structure: the device slots of a fast "
                                       "incremental step are not a consistent picture of the factorised system (new robust and polar factors are weighted on the host, old "
                                       "factors keep stale linearisations); a batch call that plans anew (april_graph_cholesky: the second in a row, or under option batch_extend = 0) "
                                       "makes %s available", what);
    // the pack the factorised system was linearised from: this graph's, unchanged in its first inc_F entries
    auto pit = g_packs.find(g);
    if (pit == g_packs.end() || pit->second->slot != t_slot || pit->second->serial != c.fact_pack)
        return refuse(-1, "no retained factor of this graph (the param's last solver call was made with another graph, or the graph's "
                          "device copy has been dropped since)");
    GraphPack &gp = *pit->second;
    // the pack is the graph's, shared by every param that solves it: lp, Delta and the weighted slots must be the ones THIS param's
    // factorisation linearised, not what a later step, LM or GNC run or failed call of another param left there
    if (gp.lin_ctx != (const void *)&c || gp.lin_serial != c.fact_serial || gp.lin_content != gp.content_version)
        return refuse(-1, "the graph's device copy no longer holds the linearisation of this param's retained factor (another "
                          "param's solver call on the graph, an april_graph_cholesky_inc_solver call, or a factor's z / W edited and evaluated since); "
                          "a batch call with this param makes %s available", what);
    const int N = c.plan.N, Fp = c.inc_F;
    if (zsize(g->nodes) != N || gp.N != N)
        return refuse(ERR_BAD_GRAPH, "the graph's node count differs from the factorised system's (nodes added since the last solver call?)");
    bool same = Fp > 0 && Fp <= gp.F && Fp <= gp.F_on_device && (int)c.pat.size() == 2 * Fp && (int)gp.is_host.size() >= Fp;
    if (same && !(c.pat_serial == gp.serial && c.pat_topo == gp.topo_version))
        for (int f = 0; f < Fp && same; f++) same = c.pat[2 * f] == gp.h_fa.p[f] && c.pat[2 * f + 1] == gp.h_fb.p[f];
    if (!same) return refuse(-1, "the graph's factors are no longer the ones the last solver call factorised (a factor's nodes or kind changed)");
    // graph factors wholly inside the factorised entries
    Fg = (int)(std::upper_bound(gp.g2p.begin(), gp.g2p.begin() + std::min<size_t>(gp.g2p.size(), (size_t)gp.Fg + 1), Fp) - gp.g2p.begin()) - 1;
    // (a caller that passes NULL sizes out by the graph it holds: never write more rows than that graph has factors)
    if (zsize(g->factors) < Fg) return refuse(ERR_BAD_GRAPH, "the graph holds fewer factors than the factorised system (factors removed since the last solver call?)");
    gpp = &gp;
    return 0;
}
static int audit_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *factors, double *out) {
    const char *who = "aprilsam_amd_factor_audit";
    if (!g || !param || !out || (factors && n < 0)) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    RetainedQuery q(who, g, param);
    GraphPack *gpp = nullptr; int Fg = 0;
    if (int rc = q.admit()) return rc;
    if (int rc = q.linearisation("the audit", gpp, Fg)) return rc;
    Context &c = q.c(); GraphPack &gp = *gpp;
    if (!factors) n = Fg;
    for (int i = 0; factors && i < n; i++)
        if (factors[i] < 0 || factors[i] >= Fg)
            return q.refuse(ERR_BAD_GRAPH, "factor index out of range of the factorised system (factors added since the last solver call?)");
    if (n == 0) return 0;
    std::vector<int> list((size_t)n), qa((size_t)n), qb((size_t)n);
    int off = 0;
    for (int i = 0; i < n; i++) {
        const int gi = factors ? factors[i] : i, p = gp.g2p[gi];
        // (host-evaluated: foreign types and cliques of more than two nodes have no slot, and user code is not called back)
        // (a dense Gaussian factor's slot holds no z / W either: DESIGN.md section 24)
        const bool ok = gp.g2p[gi + 1] - p == 1 && !gp.is_host[p] && gp.h_fa.p[p] >= 0 && !(gi < (int)gp.gs_of.size() && gp.gs_of[gi] >= 0);
        list[i] = ok ? p : -1; qa[i] = ok ? gp.h_fa.p[p] : -1; qb[i] = ok ? gp.h_fb.p[p] : -1;
        off += ok ? 0 : 1;
    }
    hipStream_t s = q.stream();
    sel_ensure(c, s);
    const int *pos = view_pos(c, s);
    c.d_sel_q.need((size_t)n);
    HIPCHECK(hipMemcpyAsync(c.d_sel_q.p, list.data(), (size_t)4 * n, hipMemcpyHostToDevice, s));
    std::vector<int> fmask;
    const bool masked = fixed_query_mask(c, n, qa.data(), qb.data(), fmask);
    if (masked) {
        c.d_fx_mask.need((size_t)n);
        HIPCHECK(hipMemcpyAsync(c.d_fx_mask.p, fmask.data(), (size_t)4 * n, hipMemcpyHostToDevice, s));
    }
    c.h_cov.need((size_t)4 * n);
    hipLaunchKernelGGL(k_factor_audit, dim3((unsigned)(((long long)n * AUDIT_LANES + 255) / 256)), dim3(256), 0, s, n, (const int *)c.d_sel_q.p,
                       masked ? (const int *)c.d_fx_mask.p : (const int *)nullptr, (const int *)gp.d_fa.p, (const int *)gp.d_fb.p, (const double *)gp.d_z.p,
                       (const double *)gp.d_W.p, (const double *)gp.d_lp.p, (const double *)gp.d_dx.p,
                       c.fact_upt ? (const double *)gp.d_upt.p : (const double *)nullptr, pos, pos + q.N(),
                       (const SelFront *)c.d_sel_fd.p, (const int *)c.d_i32.p, (const double *)c.d_sigma.p, c.h_cov.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));                      // (the host lists go out of scope)
    c.sel_serial = c.fact_serial;
    memcpy(out, c.h_cov.p, (size_t)8 * 4 * n);
    return off;
}
// As marginals: a refused or failed call writes nothing, records the error and leaves plan, factor and Sigma in place.
int factor_audit(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *factors, double *out) {
    return query_guard([&] { return audit_impl(g, param, n, factors, out); });
}
