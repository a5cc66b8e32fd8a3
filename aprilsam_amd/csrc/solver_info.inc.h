// solver_info.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam, after solver_gating.inc.h.
// Contents: aprilsam_amd_logdet / aprilsam_amd_logdet_sets / aprilsam_amd_info_gain_xyt: log-determinants of the factorised system, of the
// joint marginal covariance of node sets and of I + W H Sigma H' of candidate xyt measurements (infomeasure.hip.h).  DESIGN.md section 32.
// Admission, refusals and the guard: solver_query.inc.h; the path solves, PairBook and the argument checks of the gates: solver_gating.inc.h.
// ------------------------------------------------------------------------------------------------------
static_assert(IM_SET_MAX == APRILSAM_AMD_SET_MAX, "k_logdet_blocks's LDS is sized for the header's limit");

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

// CSR lists of 1 .. cap entries: null for a well-formed one, else what is wrong with it
static const char *csr_fault(int n, const int *ptr, int cap) {
    if (ptr[0] != 0) return "the offsets do not start at 0";
    for (int h = 0; h < n; h++) {
        const long long m = (long long)ptr[h + 1] - ptr[h];
        if (m < 0) return "the offsets decrease";
        if (m < 1 || m > cap) return "a list is empty or longer than the limit";
    }
    return nullptr;
}

// the table of k_logdet_blocks / k_gate_xyt_joint and its launch behind the path solves: hyp_ptr | tab_ptr | entries (per entries per lower
// block, made by `entry(i, j, e)` for the positions i >= j of one list in the call's arrays); in: the candidates' 18 doubles, or empty (sets).  Returns the
// number of lists with a pivot that was not positive; `out` receives the n prefixes.
template <class Entry>
static int info_blocks(RetainedQuery &q, PairBook &B, int n_hyp, const int *hyp_ptr, int per, const std::vector<double> &in, double *out, Entry entry) {
    Context &c = q.c();
    PathState &S = c.ps;
    const int n = hyp_ptr[n_hyp], np = B.n();
    std::vector<int> tab((size_t)2 * (n_hyp + 1));
    long long nT = 0;
    for (int h = 0; h < n_hyp; h++) {
        const long long m = hyp_ptr[h + 1] - hyp_ptr[h];
        tab[h] = hyp_ptr[h]; tab[(size_t)n_hyp + 1 + h] = (int)nT; nT += per * m * (m + 1) / 2;
        if (nT > 0x7fffffff) fail(ERR_OOM, "the index table of %d lists does not fit", n_hyp);
    }
    tab[n_hyp] = n; tab[(size_t)2 * n_hyp + 1] = (int)nT;
    tab.reserve(tab.size() + (size_t)nT);
    for (int h = 0; h < n_hyp; h++)
        for (int i = hyp_ptr[h]; i < hyp_ptr[h + 1]; i++)
            for (int j = hyp_ptr[h]; j <= i; j++)
                for (int e = 0; e < per; e++) tab.push_back(entry(i, j, e));
    PsTail tail;
    tail.extra = (size_t)n + n_hyp;                          // the prefixes, the lists' flags
    tail.enqueue = [&](hipStream_t st) {
        S.d_jtab.need(tab.size());
        HIPCHECK(hipMemcpyAsync(S.d_jtab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        if (!in.empty()) {
            S.d_in.need(in.size());
            HIPCHECK(hipMemcpyAsync(S.d_in.p, in.data(), in.size() * 8, hipMemcpyHostToDevice, st));
        }
        double *o = S.h_out.p + (size_t)36 * np;
        const int *t = S.d_jtab.p;
        launch_info(st, k_logdet_blocks, n_hyp, t, t + n_hyp + 1, t + 2 * (n_hyp + 1), in.empty() ? (const double *)nullptr : (const double *)S.d_in.p, np,
                    (const double *)S.d_cov.p, o, o + n);
    };
    ps_run(c, q.stream(), np, B.ua.data(), B.ub.data(), nullptr, &tail);
    const double *o = S.h_out.p + (size_t)36 * np;
    memcpy(out, o, (size_t)8 * n);
    int bad = 0;
    for (int h = 0; h < n_hyp; h++) bad += o[n + h] != 0.0;
    return bad;
}

// n_sets node sets (CSR set_ptr into nodes): nodes, then unordered pairs, deduplicated across the whole call; k_logdet_blocks behind the
// blocks.  What the checks can judge without the graph comes before the device is asked for.
static int logdet_sets_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n_sets, const int *set_ptr, const int *nodes, double *out) {
    const char *who = "aprilsam_amd_logdet_sets";
    if (!g || !param || !set_ptr || !nodes || !out || n_sets < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    if (const char *why = csr_fault(n_sets, set_ptr, APRILSAM_AMD_SET_MAX)) return refuse(ERR_BAD_GRAPH, who, "set_ptr: %s (1 to %d nodes are allowed)", why, APRILSAM_AMD_SET_MAX);
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
    return info_blocks(q, B, n_sets, set_ptr, 1, std::vector<double>(), out, [&](int i, int j, int) { return B.code(ix[i], ix[j]); });
}

// n_hyp hypotheses of candidate xyt measurements without their z: aprilsam_amd_gate_xyt_joint's checks, bookkeeping and table
static int info_gain_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *qa, const int *qb, const double *W,
                          double *out) {
    const char *who = "aprilsam_amd_info_gain_xyt";
    if (!g || !param || !hyp_ptr || !qa || !qb || !W || !out || n_hyp < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    if (const char *why = csr_fault(n_hyp, hyp_ptr, APRILSAM_AMD_JOINT_MAX))
        return refuse(ERR_BAD_GRAPH, who, "hyp_ptr: %s (1 to %d candidates are allowed)", why, APRILSAM_AMD_JOINT_MAX);
    const int n = hyp_ptr[n_hyp];
    for (int i = 0; i < n; i++) {
        if (qa[i] == qb[i]) return refuse(ERR_BAD_GRAPH, who, "a candidate joins a node to itself");
        for (int k = 0; k < 9; k++) if (!std::isfinite(W[9 * (size_t)i + k])) return refuse(ERR_BAD_GRAPH, who, "a non-finite information matrix");
    }
    for (int i = 0; i < n; i++) if (!xyt_info_spd(W + 9 * (size_t)i)) return refuse(ERR_UNSUPPORTED, who, "%s", XYT_INFO_MSG);
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    if (!ps_ids_ok(q, n, qa) || !ps_ids_ok(q, n, qb)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (n_hyp == 0) return 0;
    PairBook B(n, qa, qb);
    std::vector<int> xa((size_t)n), xb((size_t)n);          // the candidates' nodes as indices into B.un
    for (int i = 0; i < n; i++) { xa[i] = B.index(qa[i]); xb[i] = B.index(qb[i]); }
    for (int i = 0; i < n; i++) B.add(xa[i], xb[i]);       // (first: every node's own block comes from a candidate's own pair)
    for (int h = 0; h < n_hyp; h++)
        for (int i = hyp_ptr[h]; i < hyp_ptr[h + 1]; i++)
            for (int j = hyp_ptr[h]; j < i; j++)
                for (int e = 0; e < 4; e++) {
                    const int x = (e & 2) ? xb[i] : xa[i], y = (e & 1) ? xb[j] : xa[j];
                    if (x != y) B.add(x, y);
                }
    std::vector<double> in((size_t)18 * n, 0.0);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < n; i++) {
        double *v = in.data() + (size_t)18 * i;
        for (int k = 0; k < 3; k++) { v[k] = ns[qa[i]]->state[k]; v[3 + k] = ns[qb[i]]->state[k]; }
        for (int k = 0; k < 9; k++) v[9 + k] = W[9 * (size_t)i + k];
    }
    return info_blocks(q, B, n_hyp, hyp_ptr, 4, in, out, [&](int i, int j, int e) {
        // i == j: the four quarters of the candidate's own pair's block, turned round if the pair is stored as (b, a)
        const int own = B.code(xa[i], xb[i]), own0 = own & ~3, sw = (own & 3) == 1 ? 0 : 3;
        return i == j ? own0 + (e ^ sw) : B.code((e & 2) ? xb[i] : xa[i], (e & 1) ? xb[j] : xa[j]);
    });
}

int logdet(april_graph_t *g, april_graph_cholesky_param_t *param, double *out) { return query_guard([&] { return logdet_impl(g, param, out); }); }
int logdet_sets(april_graph_t *g, april_graph_cholesky_param_t *param, int n_sets, const int *set_ptr, const int *nodes, double *logdet_prefix) {
    return query_guard([&] { return logdet_sets_impl(g, param, n_sets, set_ptr, nodes, logdet_prefix); });
}
int info_gain_xyt(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b, const double *W,
                  double *gain_prefix) {
    return query_guard([&] { return info_gain_impl(g, param, n_hyp, hyp_ptr, a, b, W, gain_prefix); });
}
