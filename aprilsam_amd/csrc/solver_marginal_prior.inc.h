// solver_marginal_prior.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: aprilsam_amd_marginal_prior -- the dense Gaussian that eliminating a node set M leaves on its Markov blanket B, from the
// contribution slots the param's last factorisation linearised (k_marginal_prior, gaussian.hip.h) -- and aprilsam_amd_graph_marginalize, which
// puts it into the graph as a dense Gaussian factor and takes M out.  DESIGN.md section 24.
// Admission, refusals and the guard: solver_query.inc.h (RetainedQuery); the retained linearisation: its second step (solver_audit.inc.h).
// ------------------------------------------------------------------------------------------------------
// 0 and the prior (n_keep, keep, xbar, eta, Lambda), or a refusal's code with nothing written.  `who` names the entry point in the messages
static int marginal_prior_impl(const char *who, april_graph_t *g, april_graph_cholesky_param_t *param, int m, const int *remove, int cap, int *n_keep, int *keep,
                               double *xbar, double *eta, double *Lambda) {
    if (!g || !param || !n_keep || m < 0 || (m > 0 && !remove) || cap < 0 || (cap > 0 && (!keep || !xbar || !eta || !Lambda)))
        return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    if (m == 0) { *n_keep = 0; return 0; }
    RetainedQuery q(who, g, param);
    GraphPack *gpp = nullptr; int Fg = 0;
    if (int rc = q.admit()) return rc;
    if (int rc = q.linearisation("the marginal prior", gpp, Fg)) return rc;
    Context &c = q.c(); GraphPack &gp = *gpp;
    const int N = c.plan.N, Fp = c.inc_F;
    std::vector<int> row((size_t)N, -1);              // local row: M first, in the caller's order; then B, ascending
    for (int i = 0; i < m; i++) {
        if (remove[i] < 0 || remove[i] >= N) return q.refuse(ERR_BAD_GRAPH, "node %d out of range of the factorised system (%d nodes)", remove[i], N);
        if (row[remove[i]] >= 0) return q.refuse(ERR_BAD_GRAPH, "node %d is listed twice", remove[i]);
        row[remove[i]] = i;
    }
    // F_M from the pinned mirrors: the packed entries with an endpoint in M, ascending; B: their other endpoints
    std::vector<int> ent, B;
    for (int f = 0; f < Fp; f++) {
        const int a = gp.h_fa.p[f], b = gp.h_fb.p[f];
        if (a < 0 || !((row[a] >= 0 && row[a] < m) || (b >= 0 && row[b] >= 0 && row[b] < m))) continue;
        const int gi = gp.p2g[f];
        if (gp.g2p[gi + 1] - gp.g2p[gi] > 1)          // (its pairs that lie wholly in B would be missed)
            return q.refuse(ERR_UNSUPPORTED, "graph factor %d has more than two nodes and touches a removed node: only factors of one or two nodes may touch the "
                                             "removed set (DESIGN.md section 24)", gi);
        for (int x : { a, b }) if (x >= 0 && row[x] < 0) { row[x] = N; B.push_back(x); }      // (N: in B, row not yet known)
        ent.push_back(f); ent.push_back(a); ent.push_back(b);
    }
    std::sort(B.begin(), B.end());
    const int nb = (int)B.size();
    for (int i = 0; i < nb; i++) row[B[i]] = m + i;
    if (m + nb > MP_MAX_NODES)
        return q.refuse(ERR_UNSUPPORTED, "%d removed nodes and %d blanket nodes: more than %d together (the dense system lives in one workgroup's LDS; DESIGN.md section 24)", m, nb, MP_MAX_NODES);
    if (nb > cap)
        return q.refuse(ERR_UNSUPPORTED, "the blanket of the removed nodes has %d nodes, more than the %d that %s", nb, cap,
                        cap == GS_MAX ? "a dense Gaussian factor holds (APRILSAM_AMD_GAUSSIAN_MAX_NODES)" : "the caller made room for (cap)");
    for (const std::vector<int> *fx : { &c.fact_fixed, &gp.fx_nodes })
        for (int i : *fx)
            if (i >= 0 && i < N && row[i] >= 0)
                return q.refuse(ERR_UNSUPPORTED, "node %d is fixed and lies in the removed set or its blanket: its slots are masked (DESIGN.md section 20)", i);
    const int nE = (int)ent.size() / 3;
    for (int e = 0; e < nE; e++) { ent[3 * e + 1] = row[ent[3 * e + 1]]; ent[3 * e + 2] = ent[3 * e + 2] >= 0 ? row[ent[3 * e + 2]] : -1; }
    hipStream_t s = q.stream();
    struct Bufs { DBuf<int> ent, keep, bad; DBuf<double> out; ~Bufs() { ent.release(); keep.release(); bad.release(); out.release(); } } d;
    const int b3 = 3 * nb, n3 = 3 * (m + nb);
    const size_t n_out = (size_t)2 * b3 + (size_t)b3 * b3;
    d.ent.need(std::max<size_t>(1, ent.size())); d.keep.need(std::max(1, nb)); d.bad.need(2); d.out.need(std::max<size_t>(1, n_out));
    if (nE) HIPCHECK(hipMemcpyAsync(d.ent.p, ent.data(), ent.size() * 4, hipMemcpyHostToDevice, s));
    if (nb) HIPCHECK(hipMemcpyAsync(d.keep.p, B.data(), (size_t)4 * nb, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(d.bad.p, 0, 8, s));
    static std::once_flag once[MAX_SLOTS];            // (function attributes are kept per device)
    std::call_once(once[physical_device(t_slot) % MAX_SLOTS], [] { allow_full_lds(k_marginal_prior); });
    hipLaunchKernelGGL(k_marginal_prior, dim3(1), dim3(MP_THREADS), (size_t)8 * (n3 + 1) * (n3 + 1), s, nE, (const int *)d.ent.p, m, nb, (const int *)d.keep.p,
                       (const unsigned char *)c.d_swap.p, c.dp.slot_blk, c.dp.slot_rhs, (const double *)c.d_H.p, (const double *)gp.d_lp.p, d.out.p, d.bad.p);
    HIPCHECK(hipGetLastError());
    int bad[2] = { 0, 0 };
    std::vector<double> out(std::max<size_t>(1, n_out));
    HIPCHECK(hipMemcpyAsync(bad, d.bad.p, 8, hipMemcpyDeviceToHost, s));
    if (n_out) HIPCHECK(hipMemcpyAsync(out.data(), d.out.p, n_out * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (bad[0])         // (-2; a query: the param keeps its factorisation, which this block is only a part of)
        return q.refuse(ERR_NOT_SPD, "a pivot was not positive (scalar row %d of the removed nodes' block: node %d): the factors that touch the removed nodes do "
                                     "not determine them (information matrix of the removed block not positive definite); nothing written", bad[1], remove[bad[1] / 3]);
    *n_keep = nb;
    if (nb == 0) return 0;
    memcpy(keep, B.data(), (size_t)4 * nb);
    memcpy(xbar, out.data(), (size_t)8 * b3); memcpy(eta, out.data() + b3, (size_t)8 * b3); memcpy(Lambda, out.data() + 2 * b3, (size_t)8 * b3 * b3);
    return 0;
}
int marginal_prior(april_graph_t *g, april_graph_cholesky_param_t *param, int m, const int *remove, int cap, int *n_keep, int *keep, double *xbar, double *eta, double *Lambda) {
    return query_guard([&] { return marginal_prior_impl("aprilsam_amd_marginal_prior", g, param, m, remove, cap, n_keep, keep, xbar, eta, Lambda); });
}
// All or nothing: the prior is computed and its factor made before the graph is touched.  Returns the new factor's index, 0 with no factor
// when the blanket is empty, or the refusal's code
int graph_marginalize(april_graph_t *g, april_graph_cholesky_param_t *param, int m, const int *remove, int *new_index) {
    const char *who = "aprilsam_amd_graph_marginalize";
    int nb = 0, keep[GS_MAX];
    std::vector<double> xbar(GS_ROWS), eta(GS_ROWS), L(GS_LSZ);
    const int rc = query_guard([&] { return marginal_prior_impl(who, g, param, m, remove, GS_MAX, &nb, keep, xbar.data(), eta.data(), L.data()); });
    if (rc) return rc;
    if (m == 0) {
        if (new_index) for (int i = 0, N = zsize(g->nodes); i < N; i++) new_index[i] = i;
        return 0;
    }
    april_graph_factor_t *f = nullptr;
    if (nb > 0) {
        f = aprilsam_amd_factor_gaussian_create(nb, keep, xbar.data(), eta.data(), L.data());
        if (!f) return refuse(ERR_UNSUPPORTED, who, "the marginal prior's Lambda is not positive semi-definite to rounding (an ill-conditioned "
                                                    "removed block?); the graph is untouched");
    }
    std::vector<int> idx((size_t)zsize(g->nodes));
    if (const int rr = aprilsam_amd_graph_remove_nodes(g, m, remove, idx.data())) {      // (cannot fail after the prior's own checks; the graph is untouched if it does)
        if (f) f->destroy(f);
        return rr;
    }
    if (new_index) memcpy(new_index, idx.data(), idx.size() * 4);
    drop_context(param);                              // (plan and retained factor describe the graph before the edit: the next call plans the smaller one)
    if (!f) return 0;
    for (int i = 0; i < nb; i++) f->nodes[i] = idx[f->nodes[i]];
    aprilsam_amd_graph_add_factor(g, f);
    return zsize(g->factors) - 1;
}
