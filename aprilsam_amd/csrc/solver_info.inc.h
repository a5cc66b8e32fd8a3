// solver_info.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam, after solver_gating.inc.h.
// Contents: aprilsam_amd_logdet / aprilsam_amd_logdet_sets / aprilsam_amd_info_gain_xyt: log-determinants of the factorised system, of the
// joint marginal covariance of node sets and of I + W H Sigma H' of candidate xyt measurements (infomeasure.hip.h).  DESIGN.md section 32.
// Admission, refusals and the guard: solver_query.inc.h; the path solves, the books of pairs, the candidate checks and the frame's driver (block_lists_behind_paths): solver_gating.inc.h.
// ------------------------------------------------------------------------------------------------------
static_assert(IM_SET_MAX == APRILSAM_AMD_SET_MAX, "the frame's LDS is sized for the header's limit");

// ln det of the factorised system: one entry per (front, chunk of own columns) of the view, fronts and chunks ascending
static int logdet_impl(april_graph_t *g, april_graph_cholesky_param_t *param, double *out) {
    const char *who = "aprilsam_amd_logdet";
    if (!param || !out) return refuse(ERR_BAD_GRAPH, who, "null argument");
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    const FactorView &V = factor_view(c);
    PathState &S = c.ps;
    hipStream_t s = q.stream();
    S.h_ld.need(2);
    if (S.ld_gen != V.gen) {
        std::vector<LdEnt> ent;
        for (const SelFront &F : V.fr)
            for (int c0 = 0; c0 < F.s; c0 += LD_CHUNK) ent.push_back(LdEnt{ F.off + (long long)c0 * (F.R + 1), F.R + 1, std::min(LD_CHUNK, F.s - c0) });
        if (ent.size() > (size_t)0x7fffffff) fail(ERR_OOM, "more chunks of own columns than one launch can hold");
        S.ld_gen = -1;
        S.d_ldent.need(std::max<size_t>(1, ent.size())); S.d_ldpart.need(std::max<size_t>(1, ent.size())); S.d_ldbad.need(std::max<size_t>(1, ent.size()));
        if (!ent.empty()) HIPCHECK(hipMemcpyAsync(S.d_ldent.p, ent.data(), ent.size() * sizeof(LdEnt), hipMemcpyHostToDevice, s));
        HIPCHECK(hipStreamSynchronize(s));                  // (the host table goes out of scope)
        S.ld_n = (int)ent.size(); S.ld_gen = V.gen;
    }
    launch_info(s, S.ld_n, (const LdEnt *)S.d_ldent.p, (const double *)c.d_pool.p, S.d_ldpart.p, S.d_ldbad.p, S.h_ld.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    if (S.h_ld.p[1] != 0.0) fail(ERR_INTERNAL, "%s: %.0f diagonal entries of the retained factor are not positive and finite", who, S.h_ld.p[1]);
    *out = S.h_ld.p[0];
    return 0;
}

// n_sets node sets (CSR set_ptr into nodes): nodes, then unordered pairs, deduplicated across the whole call; the frame with SetLogdet behind the
// blocks.  What the checks can judge without the graph comes before the device is asked for.
static int logdet_sets_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n_sets, const int *set_ptr, const int *nodes, double *out) {
    const char *who = "aprilsam_amd_logdet_sets";
    if (!g || !param || !set_ptr || !nodes || !out || n_sets < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    if (int rc = csr_refusal(who, "set_ptr", n_sets, set_ptr, APRILSAM_AMD_SET_MAX)) return rc;
    for (int h = 0; h < n_sets; h++)
        for (int i = set_ptr[h]; i < set_ptr[h + 1]; i++)
            for (int j = set_ptr[h]; j < i; j++)
                if (nodes[i] == nodes[j]) return refuse(ERR_BAD_GRAPH, who, "set %d names node %d twice", h, nodes[i]);
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    const int n = set_ptr[n_sets];
    if (!ps_ids_ok(q, n, nodes)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (n_sets == 0) return 0;
    PairBook B(n, nodes, nullptr);
    std::vector<int> ix((size_t)n);
    for (int i = 0; i < n; i++) ix[i] = B.index(nodes[i]);
    for (int h = 0; h < n_sets; h++)
        for (int i = set_ptr[h]; i < set_ptr[h + 1]; i++)
            for (int j = set_ptr[h]; j < i; j++) B.add(ix[i], ix[j]);
    for (int i = 0; i < n; i++) if (B.code(ix[i], ix[i]) < 0) B.add(ix[i], ix[i]);          // (a node that only ever stands alone)
    return block_lists_behind_paths<SetLogdet>(q, B, n_sets, set_ptr, std::vector<double>(), out, nullptr, [&](int i, int j, int *e) { *e = B.code(ix[i], ix[j]); });
}

// n_hyp hypotheses of candidate xyt measurements without their z: aprilsam_amd_gate_xyt_joint's checks and book, the frame with InfoGain
static int info_gain_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *qa, const int *qb, const double *W,
                          double *out) {
    const char *who = "aprilsam_amd_info_gain_xyt";
    if (!g || !param || !hyp_ptr || !qa || !qb || !W || !out || n_hyp < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    if (int rc = csr_refusal(who, "hyp_ptr", n_hyp, hyp_ptr, APRILSAM_AMD_JOINT_MAX)) return rc;
    const int n = hyp_ptr[n_hyp];
    for (int i = 0; i < n; i++)
        if (const char *why = xyt_candidate_fault(qa[i], qb[i], nullptr, W + 9 * (size_t)i)) return refuse(ERR_BAD_GRAPH, who, "%s", why);
    if (!xyt_infos_spd(n, W)) return refuse(ERR_UNSUPPORTED, who, "%s", XYT_INFO_MSG);
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    if (!ps_ids_ok(q, n, qa) || !ps_ids_ok(q, n, qb)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (n_hyp == 0) return 0;
    HypBook B(n_hyp, hyp_ptr, qa, qb);
    return block_lists_behind_paths<InfoGain>(q, B, n_hyp, hyp_ptr, xyt_candidates_pack(g, n, qa, qb, nullptr, W), out, nullptr,
                                              [&](int i, int j, int *e) { B.entries(i, j, e); });
}

int logdet(april_graph_t *g, april_graph_cholesky_param_t *param, double *out) { return query_guard([&] { return logdet_impl(g, param, out); }); }
int logdet_sets(april_graph_t *g, april_graph_cholesky_param_t *param, int n_sets, const int *set_ptr, const int *nodes, double *logdet_prefix) {
    return query_guard([&] { return logdet_sets_impl(g, param, n_sets, set_ptr, nodes, logdet_prefix); });
}
int info_gain_xyt(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b, const double *W,
                  double *gain_prefix) {
    return query_guard([&] { return info_gain_impl(g, param, n_hyp, hyp_ptr, a, b, W, gain_prefix); });
}
