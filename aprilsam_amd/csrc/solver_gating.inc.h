// solver_gating.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: aprilsam_amd_marginals_joint_any / aprilsam_amd_gate_xyt: joint covariances of any pose pairs from the retained factor
// by triangular solves along assembly-tree paths (pathsolve.hip.h), and the Mahalanobis gating of candidate xyt measurements.
// DESIGN.md section 13.  aprilsam_amd_marginals_set / aprilsam_amd_gate_xyt_joint: the dense joint covariance of a node set and the joint
// compatibility gating of closure hypotheses (jointgate.hip.h).  DESIGN.md section 29.  aprilsam_amd_gate_polar / aprilsam_amd_associate_polar:
// the gate for range / bearing / range-bearing measurements, and their nearest-neighbour association against landmarks (polargate.hip.h).
// DESIGN.md section 21.
// Admission, refusals, the guard and the structure the factor lives in: solver_query.inc.h (RetainedQuery, FactorView).
// ------------------------------------------------------------------------------------------------------
// doubles of work buffer node q's three columns take: 3 (s + u) summed over its path
static long long ps_path_doubles(const FactorView &V, int q) {
    long long d = 0;
    for (int t = V.i32[V.N + V.i32[q]]; t >= 0; t = V.fr[t].parent) d += 3ll * (V.fr[t].s + V.fr[t].u);
    return d;
}

// One chunk: the columns of `nodes` solved along their paths, then the joint blocks of the pairs (ja, jb) (indices into nodes) into
// output slots out0, out0 + 1, ...: device S.d_cov and pinned S.h_out.
static void ps_chunk(Context &c, hipStream_t s, const std::vector<int> &nodes, const std::vector<int2> &pj, int out0) {
    PathState &S = c.ps;
    const FactorView &V = c.view;                               // (ps_run has made it current)
    const std::vector<SelFront> &fr = V.fr;
    const int N = V.N, nn = (int)nodes.size();
    std::vector<int> pbeg((size_t)nn + 1, 0), pfr;              // the fronts on each node's path, its own front first
    for (int j = 0; j < nn; j++) {
        for (int t = V.i32[N + V.i32[nodes[j]]]; t >= 0; t = fr[t].parent) pfr.push_back(t);
        pbeg[j + 1] = (int)pfr.size();
    }
    // records: the fronts the columns pass through, deepest level first (a parent's record comes after its children's)
    std::vector<int> touched;
    for (int t : pfr) if (S.rec[t] < 0) { S.rec[t] = 0; touched.push_back(t); }
    std::sort(touched.begin(), touched.end(), [&](int x, int y) { return V.depth[x] != V.depth[y] ? V.depth[x] > V.depth[y] : x < y; });
    const int nr = (int)touched.size();
    for (int r = 0; r < nr; r++) S.rec[touched[r]] = r;
    // the nodes through each record, in node-list order: slot[e] = index of path entry e's node among its front's nodes
    std::vector<int> m((size_t)nr, 0), slot(pfr.size());
    for (size_t e = 0; e < pfr.size(); e++) slot[e] = m[S.rec[pfr[e]]]++;
    std::vector<PsFront> rec((size_t)nr);
    std::vector<int> cbeg((size_t)nr + 1, 0);
    long long used = 0;
    for (int r = 0; r < nr; r++) {
        const SelFront &F = fr[touched[r]];
        PsFront &R = rec[r] = ps_front(F, used, 3 * m[r], F.parent >= 0 ? S.rec[F.parent] : -1, cbeg[r]);
        if (F.parent >= 0 && R.parent < 0) fail(ERR_INTERNAL, "aprilsam_amd_marginals_joint_any: a path leaves the tree");
        cbeg[r + 1] = cbeg[r] + R.ncol;
        used += (long long)(F.s + F.u) * R.ncol;
    }
    std::vector<int> cmap((size_t)std::max(cbeg[nr], 1), -1);
    std::vector<long long> at((size_t)3 * nn);
    std::vector<PsPath> path(pfr.size());
    for (int j = 0; j < nn; j++) {
        for (int e = pbeg[j]; e < pbeg[j + 1]; e++) {
            const PsFront &R = rec[S.rec[pfr[e]]];
            const int ld = R.s + R.u;
            path[e] = PsPath{ R.buf + 3ll * slot[e] * ld, ld, R.s };
            if (e + 1 < pbeg[j + 1])
                for (int k = 0; k < 3; k++) cmap[R.cmap + 3 * slot[e] + k] = 3 * slot[e + 1] + k;
        }
        const int e0 = pbeg[j], p = V.i32[nodes[j]];
        const SelFront &F = fr[pfr[e0]];
        const PsFront &R = rec[S.rec[pfr[e0]]];
        const int ld = R.s + R.u, l = 3 * (p - F.first);
        if (l < 0 || l + 3 > F.s) fail(ERR_INTERNAL, "aprilsam_amd_marginals_joint_any: node %d is not among its front's own rows", nodes[j]);
        for (int k = 0; k < 3; k++) at[3 * j + k] = R.buf + (3ll * slot[e0] + k) * ld + l + k;
    }
    std::vector<PsPair> pairs(pj.size());
    for (size_t i = 0; i < pj.size(); i++) {
        const int ja = pj[i].x, jb = pj[i].y, na = pbeg[ja + 1] - pbeg[ja], nb = pbeg[jb + 1] - pbeg[jb];
        int nc = 0;
        while (nc < std::min(na, nb) && pfr[pbeg[ja + 1] - 1 - nc] == pfr[pbeg[jb + 1] - 1 - nc]) nc++;
        pairs[i] = PsPair{ pbeg[ja], na, pbeg[jb], nb, nc, out0 + (int)i };
    }
    // work entries, level by level
    struct Lev { Span trsm, gemm; };
    std::vector<Lev> lev;
    std::vector<int4> ent;
    for (int r0 = 0; r0 < nr; ) {
        int r1 = r0;
        while (r1 < nr && V.depth[touched[r1]] == V.depth[touched[r0]]) r1++;
        Lev L;
        L.trsm = span_of(ent, [&] { for (int r = r0; r < r1; r++) for (int y = 0; y * SEL_T < rec[r].ncol; y++) ent.push_back(int4{ r, y, 0, 0 }); });
        L.gemm = span_of(ent, [&] {
            for (int r = r0; r < r1; r++)
                if (rec[r].parent >= 0)
                    for (int y = 0; y * SEL_T < rec[r].ncol; y++) for (int i = 0; i * SEL_T < rec[r].u; i++) ent.push_back(int4{ r, i, y, 0 });
        });
        lev.push_back(L);
        r0 = r1;
    }
    for (int t : touched) S.rec[t] = -1;
    if (ent.empty()) ent.push_back(int4{ 0, 0, 0, 0 });
    S.d_fr.need(std::max<size_t>(1, rec.size())); S.d_ent.need(ent.size()); S.d_cmap.need(cmap.size()); S.d_at.need(at.size());
    S.d_path.need(path.size()); S.d_pair.need(pairs.size()); S.d_buf.need((size_t)std::max(used, 1ll));
    S.peak_doubles = std::max(S.peak_doubles, used);
    HIPCHECK(hipMemcpyAsync(S.d_fr.p, rec.data(), rec.size() * sizeof(PsFront), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(S.d_ent.p, ent.data(), ent.size() * sizeof(int4), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(S.d_cmap.p, cmap.data(), cmap.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(S.d_at.p, at.data(), at.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(S.d_path.p, path.data(), path.size() * sizeof(PsPath), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(S.d_pair.p, pairs.data(), pairs.size() * sizeof(PsPair), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(S.d_buf.p, 0, (size_t)used * 8, s));
    const PsFront *dfr = S.d_fr.p; const int4 *de = S.d_ent.p; const double *pool = c.d_pool.p; double *buf = S.d_buf.p;
    hipLaunchKernelGGL(k_path_init, dim3((unsigned)((at.size() + 255) / 256)), dim3(256), 0, s, (int)at.size(), (const long long *)S.d_at.p, buf);
    for (const Lev &L : lev) {
        launch_waves(k_path_trsm, s, L.trsm, 1, dfr, de, pool, buf);
        launch_waves(k_path_gemm, s, L.gemm, 1, dfr, de, pool, (const int *)c.d_i32.p, (const int *)S.d_cmap.p, buf);
    }
    hipLaunchKernelGGL(k_path_gram, dim3((unsigned)pairs.size()), dim3(256), 0, s, (const PsPair *)S.d_pair.p, (const PsPath *)S.d_path.p,
                       (const double *)buf, S.d_cov.p, S.h_out.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));                      // (the host tables go out of scope; the next chunk reuses the buffers)
}

// the doubles of work buffer one chunk may take: 1 GB, or option mem_cap_mb (the limit on any single device buffer)
static long long ps_budget() {
    const long long dflt = 1ll << 27;
    return g_opt.mem_cap_mb > 0 ? std::min(dflt, ((long long)g_opt.mem_cap_mb << 20) / 8) : dflt;
}

// what a caller of ps_run runs behind the blocks (the gates, the information measures): `extra` doubles of S.h_out behind the 36 n of the
// blocks, and what enqueues its copies and its kernel on the stream, which is synchronised after it
struct PsTail { size_t extra = 0; std::function<void(hipStream_t)> enqueue; };

// joint blocks of the n pairs (qa, qb) into S.d_cov / S.h_out (36 per pair): the path solves, the mask of the fixed nodes, then the tail
static void ps_run(Context &c, hipStream_t s, int n, const int *qa, const int *qb, const PsTail *tail = nullptr) {
    const FactorView &V = factor_view(c);
    PathState &S = c.ps;
    if (S.gen != V.gen) { S.rec.assign(V.fr.size(), -1); S.node_j.assign((size_t)V.N, -1); S.gen = V.gen; }
    S.d_cov.need((size_t)36 * n);
    S.h_out.need((size_t)36 * n + (tail ? tail->extra : 0));
    const long long budget = ps_budget();
    std::vector<int> nodes; std::vector<int2> pj;
    long long used = 0;
    int first = 0;
    auto flush = [&](int end) {
        if (!pj.empty()) ps_chunk(c, s, nodes, pj, first);
        for (int q : nodes) S.node_j[q] = -1;
        nodes.clear(); pj.clear(); used = 0; first = end;
    };
    try {
    for (int i = 0; i < n; i++) {
        long long add = 0;
        if (S.node_j[qa[i]] < 0) add += ps_path_doubles(V, qa[i]);
        if (qb[i] != qa[i] && S.node_j[qb[i]] < 0) add += ps_path_doubles(V, qb[i]);
        if (!pj.empty() && used + add > budget) flush(i);
        for (int q : { qa[i], qb[i] })
            if (S.node_j[q] < 0) { S.node_j[q] = (int)nodes.size(); nodes.push_back(q); used += ps_path_doubles(V, q); }
        pj.push_back(int2{ S.node_j[qa[i]], S.node_j[qb[i]] });
    }
    flush(n);
    } catch (...) {                                         // (rec and node_j hold this call's marks: the next call sets both to -1 again)
        S.node_j.clear(); S.gen = -1;
        throw;
    }
    std::vector<int> fmask;
    if (fixed_query_mask(c, n, qa, qb, fmask)) {      // fixed nodes: their rows and columns are exact zeros before anything leaves or is gated (k_fix_cov)
        c.d_fx_mask.need((size_t)n);
        HIPCHECK(hipMemcpyAsync(c.d_fx_mask.p, fmask.data(), (size_t)4 * n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fix_cov, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, n, (const int *)c.d_fx_mask.p, 36, S.d_cov.p, S.h_out.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
    }
    if (tail) {
        tail->enqueue(s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
    }
}

// node ids against the factorised system and, for the calls that read states, the graph
static const char *const PS_RANGE_MSG = "node id out of range of the factorised system (nodes added since the last solver call?)";
static bool ps_ids_ok(const RetainedQuery &q, int n, const int *ids) {
    const int N = q.N(), Ng = zsize(q.g->nodes);
    for (int i = 0; i < n; i++) if (ids[i] < 0 || ids[i] >= N || ids[i] >= Ng) return false;
    return true;
}

static int joint_any_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, double *cov) {
    const char *who = "aprilsam_amd_marginals_joint_any";
    if (!param || !cov || !qa || !qb || n < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    const int N = q.N();
    for (int i = 0; i < n; i++)
        if (qa[i] < 0 || qa[i] >= N || qb[i] < 0 || qb[i] >= N) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (n == 0) return 0;
    ps_run(c, q.stream(), n, qa, qb);
    memcpy(cov, c.ps.h_out.p, (size_t)8 * 36 * n);
    return 0;
}

// a candidate's information matrix (3 x 3, row-major): symmetric (mirror entries equal) and positive definite: a Cholesky factorisation
static const char *const XYT_INFO_MSG = "an information matrix that is not symmetric positive definite";
static bool xyt_info_spd(const double *w) {
    bool ok = w[1] == w[3] && w[2] == w[6] && w[5] == w[7];
    const double l00 = w[0] > 0 ? sqrt(w[0]) : 0;
    ok = ok && l00 > 0;
    const double l10 = ok ? w[3] / l00 : 0, l20 = ok ? w[6] / l00 : 0, p1 = w[4] - l10 * l10;
    ok = ok && p1 > 0;
    const double l11 = ok ? sqrt(p1) : 0, l21 = ok ? (w[7] - l20 * l10) / l11 : 0, p2 = w[8] - l20 * l20 - l21 * l21;
    return ok && p2 > 0;
}

// One candidate xyt measurement between a and b (z null: without one), before its information matrix is factorised: null, or what
// ERR_BAD_GRAPH is refused for.  Every candidate of a call passes this before xyt_infos_spd judges the matrices (ERR_UNSUPPORTED, XYT_INFO_MSG)
static const char *xyt_candidate_fault(int a, int b, const double *z, const double *W) {
    if (a == b) return "a candidate joins a node to itself";
    for (int k = 0; z && k < 3; k++) if (!std::isfinite(z[k])) return "a non-finite measurement";
    for (int k = 0; k < 9; k++) if (!std::isfinite(W[k])) return "a non-finite information matrix";
    return nullptr;
}
static bool xyt_infos_spd(int n, const double *W) {
    for (int i = 0; i < n; i++) if (!xyt_info_spd(W + 9 * (size_t)i)) return false;
    return true;
}

// the candidates as the kernels take them, 18 doubles each: the states of a and b, z (or three zeros), W
static std::vector<double> xyt_candidates_pack(const april_graph_t *g, int n, const int *qa, const int *qb, const double *z, const double *W) {
    std::vector<double> in((size_t)18 * n, 0.0);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < n; i++) {
        double *v = in.data() + (size_t)18 * i;
        for (int k = 0; k < 3; k++) { v[k] = ns[qa[i]]->state[k]; v[3 + k] = ns[qb[i]]->state[k]; if (z) v[6 + k] = z[3 * (size_t)i + k]; }
        for (int k = 0; k < 9; k++) v[9 + k] = W[9 * (size_t)i + k];
    }
    return in;
}

// candidate i against the joint block of its own pair (a[i], b[i]), one path solve per candidate: k_gate_xyt behind the blocks
static int gate_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, const double *z, const double *W,
                     double *d2, double *Sout) {
    const char *who = "aprilsam_amd_gate_xyt";
    if (!g || !param || !qa || !qb || !z || !W || !d2 || n < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    for (int i = 0; i < n; i++) {
        if (!ps_ids_ok(q, 1, qa + i) || !ps_ids_ok(q, 1, qb + i)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
        if (const char *why = xyt_candidate_fault(qa[i], qb[i], z + 3 * (size_t)i, W + 9 * (size_t)i)) return q.refuse(ERR_BAD_GRAPH, "%s", why);
    }
    if (!xyt_infos_spd(n, W)) return q.refuse(ERR_UNSUPPORTED, "%s", XYT_INFO_MSG);
    if (n == 0) return 0;
    const std::vector<double> in = xyt_candidates_pack(g, n, qa, qb, z, W);
    PathState &S = c.ps;
    PsTail tail;
    tail.extra = (size_t)10 * n;                            // d2, then S
    tail.enqueue = [&](hipStream_t st) {
        S.d_in.need(in.size());
        HIPCHECK(hipMemcpyAsync(S.d_in.p, in.data(), in.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gate_xyt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const double *)S.d_in.p, (const double *)S.d_cov.p,
                           S.h_out.p + (size_t)36 * n);
    };
    ps_run(c, q.stream(), n, qa, qb, &tail);
    const double *o = S.h_out.p + (size_t)36 * n;
    memcpy(d2, o, (size_t)8 * n);
    if (Sout) memcpy(Sout, o + n, (size_t)8 * 9 * n);
    return 0;
}

// ---- node sets and joint compatibility ---------------------------------------------------------------------------
// The distinct unordered node pairs of one call, each solved once: slot s holds the 6 x 6 block of (ua[s], ub[s]) in the order it was first
// asked for.  code(x, y) = 4 slot + quarter names the 3 x 3 block S(p, q) inside it (the table entry of jointgate.hip.h's frame) for the call's distinct
// nodes p = un[x], q = un[y]: quarter 1 the pair as stored, 2 the pair the other way round, 0 / 3 a node's own block -- taken from the
// first pair that named the node.  The codes of all ordered index pairs lie in a table of nu x nu entries while the call names at most
// DENSE_MAX distinct nodes (a branch-and-bound level shares a few tens of nodes among its hypotheses: one array read per entry of the
// kernel's index table), in a hash map beyond.
static_assert(JG_MAX == APRILSAM_AMD_JOINT_MAX, "the frame's LDS is sized for the header's limit");
struct PairBook {
    static constexpr int DENSE_MAX = 1024;
    std::vector<int> un, ua, ub;                             // the distinct nodes, ascending; slot -> its pair (node ids)
    std::vector<int> dense;
    std::unordered_map<long long, int> sparse;
    // the nodes of the call: ids[0..n) and, if not null, more[0..n)
    PairBook(int n, const int *ids, const int *more) : un(ids, ids + n) {
        if (more) un.insert(un.end(), more, more + n);
        std::sort(un.begin(), un.end());
        un.erase(std::unique(un.begin(), un.end()), un.end());
        if (un.size() <= (size_t)DENSE_MAX) dense.assign(un.size() * un.size(), -1);
    }
    int index(int node) const { return (int)(std::lower_bound(un.begin(), un.end(), node) - un.begin()); }
    int code(int x, int y) const {
        if (!dense.empty()) return dense[(size_t)x * un.size() + y];
        auto it = sparse.find(((long long)x << 32) | (unsigned)y);
        return it == sparse.end() ? -1 : it->second;
    }
    void set(int x, int y, int v) {
        if (!dense.empty()) dense[(size_t)x * un.size() + y] = v;
        else sparse[((long long)x << 32) | (unsigned)y] = v;
    }
    void add(int x, int y) {
        if (code(x, y) >= 0) return;
        if (ua.size() >= (size_t)(0x7fffffff / 36)) fail(ERR_OOM, "more distinct node pairs than one call can hold");
        const int s4 = 4 * (int)ua.size();
        ua.push_back(un[x]); ub.push_back(un[y]);
        if (x != y) { set(x, y, s4 + 1); set(y, x, s4 + 2); }
        if (code(x, x) < 0) set(x, x, s4);
        if (code(y, y) < 0) set(y, y, s4 + 3);
    }
    int n() const { return (int)ua.size(); }
};

// dense joint covariance of the k listed nodes: every distinct node solved once, every distinct unordered pair through k_path_gram once
static int marginals_set_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int k, const int *nodes, double *cov) {
    const char *who = "aprilsam_amd_marginals_set";
    if (!param || k < 0 || (k > 0 && (!nodes || !cov))) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    const int N = q.N();
    for (int i = 0; i < k; i++) if (nodes[i] < 0 || nodes[i] >= N) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (k == 0) return 0;
    PairBook B(k, nodes, nullptr);
    const int nu = (int)B.un.size();
    if (nu == 1) B.add(0, 0);
    for (int x = 0; x < nu; x++) for (int y = x + 1; y < nu; y++) B.add(x, y);
    ps_run(c, q.stream(), B.n(), B.ua.data(), B.ub.data());
    std::vector<int> ix((size_t)k);
    for (int i = 0; i < k; i++) ix[i] = B.index(nodes[i]);
    const double *o = c.ps.h_out.p;
    const size_t ld = (size_t)3 * k;
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            const int code = B.code(ix[i], ix[j]), ro = (code & 2) ? 3 : 0, co = (code & 1) ? 3 : 0;
            const double *blk = o + (size_t)36 * (code >> 2);
            for (int x = 0; x < 3; x++) for (int y = 0; y < 3; y++) cov[(3 * i + x) * ld + 3 * j + y] = blk[6 * (ro + x) + co + y];
        }
    return 0;
}

// CSR lists of 1 .. cap entries: 0 for well-formed offsets, else ERR_BAD_GRAPH refused for `who`, naming the offsets (`what`), the first
// list at fault and its length
static int csr_refusal(const char *who, const char *what, int n, const int *ptr, int cap) {
    if (ptr[0] != 0) return refuse(ERR_BAD_GRAPH, who, "%s does not start at 0", what);
    for (int h = 0; h < n; h++) {
        const long long m = (long long)ptr[h + 1] - ptr[h];
        if (m < 0) return refuse(ERR_BAD_GRAPH, who, "%s decreases at list %d", what, h);
        if (m < 1 || m > cap) return refuse(ERR_BAD_GRAPH, who, "%s: list %d has %lld entries (1 to %d are allowed)", what, h, m, cap);
    }
    return 0;
}

// The book of a call over hypotheses of candidates (qa[i], qb[i]), CSR hyp_ptr: the candidates' own pairs first (every node's own block comes
// from a candidate's own pair), then the four cross pairs of every two candidates of a hypothesis
struct HypBook : PairBook {
    std::vector<int> xa, xb;                                 // the candidates' nodes as indices into un
    HypBook(int n_hyp, const int *hyp_ptr, const int *qa, const int *qb) : PairBook(hyp_ptr[n_hyp], qa, qb) {
        const int n = hyp_ptr[n_hyp];
        xa.resize((size_t)n); xb.resize((size_t)n);
        for (int i = 0; i < n; i++) { xa[i] = index(qa[i]); xb[i] = index(qb[i]); }
        for (int i = 0; i < n; i++) add(xa[i], xb[i]);
        for (int h = 0; h < n_hyp; h++)
            for (int i = hyp_ptr[h]; i < hyp_ptr[h + 1]; i++)
                for (int j = hyp_ptr[h]; j < i; j++)
                    for (int e = 0; e < 4; e++) {
                        const int x = (e & 2) ? xb[i] : xa[i], y = (e & 1) ? xb[j] : xa[j];
                        if (x != y) add(x, y);
                    }
    }
    // the four entries of lower block (i, j): S(a_i,a_j), S(a_i,b_j), S(b_i,a_j), S(b_i,b_j); i == j: the four quarters of the candidate's own
    // pair's block, turned round if the pair is stored as (b, a)
    void entries(int i, int j, int *out) const {
        if (i == j) {
            const int own = code(xa[i], xb[i]), own0 = own & ~3, sw = (own & 3) == 1 ? 0 : 3;
            for (int e = 0; e < 4; e++) out[e] = own0 + (e ^ sw);
        } else
            for (int e = 0; e < 4; e++) out[e] = code((e & 2) ? xb[i] : xa[i], (e & 1) ? xb[j] : xa[j]);
    }
};

// The pairs of B solved, then jointgate.hip.h's frame with rider R over the n_hyp lists behind them.  Its table: hyp_ptr | tab_ptr | R::PER
// entries per lower block, written by `entries(i, j, out)` for the positions i >= j of one list in the call's arrays; in: the candidates' 18 doubles,
// or empty; C (or null): receives the lists' matrices, 9 m^2 doubles each, one behind the other.  `out` receives the n prefixes.  Returns
// the number of lists with a pivot that was not positive
template <class R, class Entries>
static int block_lists_behind_paths(RetainedQuery &q, PairBook &B, int n_hyp, const int *hyp_ptr, const std::vector<double> &in, double *out, double *C, Entries entries) {
    Context &c = q.c();
    PathState &S = c.ps;
    const int n = hyp_ptr[n_hyp], np = B.n();
    std::vector<int> tab((size_t)2 * (n_hyp + 1));
    std::vector<long long> coff((size_t)n_hyp);
    long long nC = 0, nT = 0;
    for (int h = 0; h < n_hyp; h++) {
        const long long m = hyp_ptr[h + 1] - hyp_ptr[h];
        coff[h] = nC; nC += 9 * m * m;
        tab[h] = hyp_ptr[h]; tab[(size_t)n_hyp + 1 + h] = (int)nT; nT += R::PER * m * (m + 1) / 2;
        if (nT > 0x7fffffff) fail(ERR_OOM, "the index table of %d lists does not fit", n_hyp);
    }
    tab[n_hyp] = n; tab[(size_t)2 * n_hyp + 1] = (int)nT;
    size_t at = tab.size();
    tab.resize(at + (size_t)nT);
    for (int h = 0; h < n_hyp; h++)
        for (int i = hyp_ptr[h]; i < hyp_ptr[h + 1]; i++)
            for (int j = hyp_ptr[h]; j <= i; j++, at += R::PER) entries(i, j, tab.data() + at);
    PsTail tail;
    tail.extra = (size_t)n + n_hyp + (C ? (size_t)nC : 0);   // the prefixes, the lists' flags, the matrices
    tail.enqueue = [&](hipStream_t st) {
        S.d_jtab.need(tab.size());
        HIPCHECK(hipMemcpyAsync(S.d_jtab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        if (!in.empty()) {
            S.d_in.need(in.size());
            HIPCHECK(hipMemcpyAsync(S.d_in.p, in.data(), in.size() * 8, hipMemcpyHostToDevice, st));
        }
        if (C) {
            S.d_joff.need(coff.size());
            HIPCHECK(hipMemcpyAsync(S.d_joff.p, coff.data(), coff.size() * 8, hipMemcpyHostToDevice, st));
        }
        double *o = S.h_out.p + (size_t)36 * np;
        const int *t = S.d_jtab.p;
        launch_block_chol<R>(st, n_hyp, t, t + n_hyp + 1, t + 2 * (n_hyp + 1), np, (const double *)S.d_cov.p, o, o + n,
                             in.empty() ? (const double *)nullptr : (const double *)S.d_in.p, C ? (const long long *)S.d_joff.p : (const long long *)nullptr,
                             C ? o + n + n_hyp : (double *)nullptr);
    };
    ps_run(c, q.stream(), np, B.ua.data(), B.ub.data(), &tail);
    const double *o = S.h_out.p + (size_t)36 * np;
    memcpy(out, o, (size_t)8 * n);
    if (C) memcpy(C, o + n + n_hyp, (size_t)8 * nC);
    int bad = 0;
    for (int h = 0; h < n_hyp; h++) bad += o[n + h] != 0.0;
    return bad;
}

// n_hyp hypotheses (CSR hyp_ptr into a / b / z / W): nodes, then unordered node pairs, deduplicated across the whole call; the frame with
// JointGate behind the blocks.  What the checks can judge without the graph comes before the device is asked for.
static int gate_joint_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *qa, const int *qb, const double *z,
                           const double *W, double *d2, double *Cout) {
    const char *who = "aprilsam_amd_gate_xyt_joint";
    if (!g || !param || !hyp_ptr || !qa || !qb || !z || !W || !d2 || n_hyp < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    if (int rc = csr_refusal(who, "hyp_ptr", n_hyp, hyp_ptr, APRILSAM_AMD_JOINT_MAX)) return rc;
    const int n = hyp_ptr[n_hyp];
    for (int i = 0; i < n; i++)
        if (const char *why = xyt_candidate_fault(qa[i], qb[i], z + 3 * (size_t)i, W + 9 * (size_t)i)) return refuse(ERR_BAD_GRAPH, who, "%s", why);
    if (!xyt_infos_spd(n, W)) return refuse(ERR_UNSUPPORTED, who, "%s", XYT_INFO_MSG);
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    if (!ps_ids_ok(q, n, qa) || !ps_ids_ok(q, n, qb)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (n_hyp == 0) return 0;
    HypBook B(n_hyp, hyp_ptr, qa, qb);
    return block_lists_behind_paths<JointGate>(q, B, n_hyp, hyp_ptr, xyt_candidates_pack(g, n, qa, qb, z, W), d2, Cout,
                                               [&](int i, int j, int *out) { B.entries(i, j, out); });
}

// ---- polar gates ----------------------------------------------------------------------------------------------
// n candidates (kind, z, W) between a[i] and b[i]: every DISTINCT pair (a, b) is solved once, k_gate_polar reads a candidate's block through
// its pair index.  What the checks can judge without the graph comes before the device is asked for.
static int gate_polar_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, const int *kind, const double *z,
                           const double *W, double *d2, double *Sout) {
    const char *who = "aprilsam_amd_gate_polar", *why = nullptr;
    if (!g || !param || !qa || !qb || !kind || !z || !W || !d2 || n < 0) return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    for (int i = 0; i < n; i++) if (qa[i] == qb[i]) return refuse(ERR_BAD_GRAPH, who, "a candidate joins a node to itself");
    if (int rc = polar_gate_args(n, kind, z, W, &why)) return refuse(rc, who, "%s", why);
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    if (!ps_ids_ok(q, n, qa) || !ps_ids_ok(q, n, qb)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (n == 0) return 0;
    std::vector<int> ua, ub, pidx((size_t)n);
    std::unordered_map<long long, int> seen;
    for (int i = 0; i < n; i++) {
        auto r = seen.emplace(((long long)qa[i] << 32) | (unsigned)qb[i], (int)ua.size());
        if (r.second) { ua.push_back(qa[i]); ub.push_back(qb[i]); }
        pidx[i] = r.first->second;
    }
    const int np = (int)ua.size();
    std::vector<double> in((size_t)PG_IN * n, 0.0);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < n; i++) {
        double *q = in.data() + (size_t)PG_IN * i;
        const int m = polar_rows(kind[i]);
        for (int k = 0; k < 3; k++) { q[k] = ns[qa[i]]->state[k]; q[3 + k] = ns[qb[i]]->state[k]; }
        q[6] = kind[i];
        for (int k = 0; k < m; k++) q[7 + k] = z[2 * i + k];
        for (int k = 0; k < m * m; k++) q[9 + k] = W[4 * i + k];
    }
    PathState &S = c.ps;
    PsTail tail;
    tail.extra = (size_t)6 * n;
    tail.enqueue = [&](hipStream_t st) {
        S.d_in.need(in.size()); S.d_pidx.need((size_t)n);
        HIPCHECK(hipMemcpyAsync(S.d_in.p, in.data(), in.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(S.d_pidx.p, pidx.data(), (size_t)4 * n, hipMemcpyHostToDevice, st));
        launch_polar_gate(st, k_gate_polar, n, false, n, (const double *)S.d_in.p, (const int *)S.d_pidx.p, (const double *)S.d_cov.p, S.h_out.p + (size_t)36 * np);
    };
    ps_run(c, q.stream(), np, ua.data(), ub.data(), &tail);
    const double *o = S.h_out.p + (size_t)36 * np;
    memcpy(d2, o, (size_t)8 * n);
    if (Sout) memcpy(Sout, o + n, (size_t)8 * 4 * n);
    int unavailable = 0;
    for (int i = 0; i < n; i++) unavailable += o[(size_t)5 * n + i] == 0.0;
    return unavailable;
}

// m observations (kind, z, W) made from `observer` against the L nodes `landmarks`: the L pairs (observer, landmarks[l]) are solved once,
// k_associate_polar gates every observation against every pair and reduces on the device.
static int associate_polar_impl(april_graph_t *g, april_graph_cholesky_param_t *param, int observer, int m, const int *kind, const double *z, const double *W,
                                int L, const int *landmarks, double gate1, double gate2, double *d2, int *best, double *d2_best, double *d2_second) {
    const char *who = "aprilsam_amd_associate_polar", *why = nullptr;
    if (!g || !param || !kind || !z || !W || !landmarks || !best || !d2_best || !d2_second || m < 0 || L < 0)
        return refuse(ERR_BAD_GRAPH, who, "null argument or negative count");
    for (int l = 0; l < L; l++) if (landmarks[l] == observer) return refuse(ERR_BAD_GRAPH, who, "the observer is among the landmarks");
    if (!std::isfinite(gate1) || !std::isfinite(gate2)) return refuse(ERR_BAD_GRAPH, who, "a non-finite gate");
    if (int rc = polar_gate_args(m, kind, z, W, &why)) return refuse(rc, who, "%s", why);
    RetainedQuery q(who, g, param);
    if (int rc = q.admit()) return rc;
    Context &c = q.c();
    if (!ps_ids_ok(q, 1, &observer) || !ps_ids_ok(q, L, landmarks)) return q.refuse(ERR_BAD_GRAPH, "%s", PS_RANGE_MSG);
    if (m == 0) return 0;
    if (L == 0) {
        for (int i = 0; i < m; i++) { best[i] = -1; d2_best[i] = INFINITY; d2_second[i] = INFINITY; }
        return 0;
    }
    const std::vector<int> qa((size_t)L, observer);
    std::vector<double> in((size_t)PG_OBS * m + 3 + (size_t)3 * L, 0.0);       // the observations, then the states: the observer's, the landmarks'
    for (int i = 0; i < m; i++) {
        double *q = in.data() + (size_t)PG_OBS * i;
        const int r = polar_rows(kind[i]);
        q[0] = kind[i];
        for (int k = 0; k < r; k++) q[1 + k] = z[2 * i + k];
        for (int k = 0; k < r * r; k++) q[3 + k] = W[4 * i + k];
    }
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    double *st = in.data() + (size_t)PG_OBS * m;
    for (int k = 0; k < 3; k++) st[k] = ns[observer]->state[k];
    for (int l = 0; l < L; l++) for (int k = 0; k < 3; k++) st[3 + 3 * (size_t)l + k] = ns[landmarks[l]]->state[k];
    PathState &S = c.ps;
    const size_t nmat = d2 ? (size_t)m * L : 0;
    PsTail tail;
    tail.extra = nmat + (size_t)3 * m;             // the matrix, d2_best, d2_second, then (best, unavailable) as two ints per observation
    tail.enqueue = [&](hipStream_t sq) {
        S.d_in.need(in.size());
        HIPCHECK(hipMemcpyAsync(S.d_in.p, in.data(), in.size() * 8, hipMemcpyHostToDevice, sq));
        double *o = S.h_out.p + (size_t)36 * L;
        launch_polar_gate(sq, k_associate_polar, m, true, L, (const double *)S.d_in.p, (const double *)S.d_in.p + (size_t)PG_OBS * m, (const double *)S.d_cov.p,
                          gate1, gate2, d2 ? o : (double *)nullptr, (int2 *)(o + nmat + (size_t)2 * m), o + nmat, o + nmat + m);
    };
    ps_run(c, q.stream(), L, qa.data(), landmarks, &tail);
    const double *o = S.h_out.p + (size_t)36 * L;
    if (d2) memcpy(d2, o, 8 * nmat);
    memcpy(d2_best, o + nmat, (size_t)8 * m);
    memcpy(d2_second, o + nmat + m, (size_t)8 * m);
    const int2 *res = (const int2 *)(o + nmat + (size_t)2 * m);
    long long unavailable = 0;
    for (int i = 0; i < m; i++) { best[i] = res[i].x; unavailable += res[i].y; }
    return (int)std::min<long long>(unavailable, 0x7fffffff);
}

int marginals_joint_any(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, double *cov) {
    return query_guard([&] { return joint_any_impl(g, param, n, a, b, cov); });
}
int gate_xyt(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, const double *z, const double *W, double *d2, double *S) {
    return query_guard([&] { return gate_impl(g, param, n, a, b, z, W, d2, S); });
}
int marginals_set(april_graph_t *g, april_graph_cholesky_param_t *param, int k, const int *nodes, double *cov) {
    return query_guard([&] { return marginals_set_impl(g, param, k, nodes, cov); });
}
int gate_xyt_joint(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b, const double *z,
                   const double *W, double *d2_prefix, double *C) {
    return query_guard([&] { return gate_joint_impl(g, param, n_hyp, hyp_ptr, a, b, z, W, d2_prefix, C); });
}
int gate_polar(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, const int *kind, const double *z, const double *W,
               double *d2, double *S) {
    return query_guard([&] { return gate_polar_impl(g, param, n, a, b, kind, z, W, d2, S); });
}
int associate_polar(april_graph_t *g, april_graph_cholesky_param_t *param, int observer, int m, const int *kind, const double *z, const double *W, int L,
                    const int *landmarks, double gate1, double gate2, double *d2, int *best, double *d2_best, double *d2_second) {
    return query_guard([&] { return associate_polar_impl(g, param, observer, m, kind, z, W, L, landmarks, gate1, gate2, d2, best, d2_best, d2_second); });
}
long long path_solve_bytes(const april_graph_cholesky_param_t *param) { return context_field(param, [](const Context &c) { return 8 * c.ps.peak_doubles; }); }
