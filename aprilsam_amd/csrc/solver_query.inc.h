// solver_query.inc.h -- part of solver.hip.cpp (ONE translation unit); included from there, inside namespace asam.
// Contents: what every consumer of the retained factor starts with: the one refusal (refuse), the one guard
// (query_guard), the session of one query (RetainedQuery: device, slot lock, the admission sequence, N, a lazily taken stream) and the one
// view of the structure the factor lives in (FactorView, built by factor_view), which the selected inversion, the path solves and the
// tree solves all read.
// ------------------------------------------------------------------------------------------------------
// nodes of the system the retained factor was made from
static int retained_N(const Context &c) { return c.fact_kind == FACT_EXTENDED ? c.inc_N : c.plan.N; }

// The refusal of a query: "<who>: <reason>" recorded for aprilsam_amd_last_error and printed; the param keeps plan and factor.  Returns
// the code.  (gate_refuse: the same for a message that is already whole -- the optimisers' argument checks use it too)
static int gate_refuse(int code, const char *msg) {
    set_last_error(code, msg); fprintf(stderr, "aprilsam_amd: ERROR %d: %s\n", code, msg); fflush(stderr); return code;
}
static int refusev(int code, const char *who, const char *fmt, va_list ap) {
    char msg[1024];
    const int k = snprintf(msg, sizeof msg, "%s: ", who);
    vsnprintf(msg + k, sizeof msg - (size_t)k, fmt, ap);
    return gate_refuse(code, msg);
}
static int refuse(int code, const char *who, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static int refuse(int code, const char *who, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt);
    const int rc = refusev(code, who, fmt, ap);
    va_end(ap);
    return rc;
}

// A query that fails only READ the param's plan and factor: unlike the solver entry points (guarded) it records the error and leaves both
// in place (the next solver call is unaffected).
template <class F> static int query_guard(F f) {
    try { return f(); }
    catch (const SolverError &e) { set_last_error(e.code, e.msg); fprintf(stderr, "aprilsam_amd: ERROR %d: %s\n", e.code, e.msg.c_str()); fflush(stderr); (void)hipGetLastError(); return e.code; }
    catch (const std::bad_alloc &) { set_last_error(ERR_OOM, "host memory exhausted (std::bad_alloc)"); return ERR_OOM; }
    catch (const std::exception &e) { set_last_error(ERR_INTERNAL, e.what()); return ERR_INTERNAL; }
}

// Fixed nodes: the consumers of the retained factor describe the system it was made from, identity blocks
// included.  A node fixed or freed since then makes that system another one: the factor is dropped, and the consumer answers as without.
static void drop_factor_if_toggled(Context &c, const april_graph_t *g) {
    if (!g || (c.fact_fixed.empty() && !fixed_ever())) return;
    std::vector<int> now;
    scan_fixed(g, now);
    if (now != c.fact_fixed) { c.have_fact = false; c.fact_kind = FACT_NONE; }
}

// One query of the retained factor.  An entry point makes its own argument checks (refuse), constructs the session -- the device, the
// slot lock -- and asks admit(): 0 and c is the param's context, or the code of a refusal that is already recorded.  A new consumer
// starts exactly so.  The stream comes from the slot's pool when stream() is first asked and goes back when the session ends: a refused
// call takes none.
struct RetainedQuery {
    const char *const who; april_graph_t *const g; april_graph_cholesky_param_t *const param;
    SlotLock lk;
    Context *cp = nullptr;
    hipStream_t s = nullptr;
    RetainedQuery(const char *who, april_graph_t *g, april_graph_cholesky_param_t *param) : who(who), g(g), param(param), lk((ensure_device(), param), g) {}
    RetainedQuery(const RetainedQuery &) = delete;
    ~RetainedQuery() { if (s) park_stream(t_slot, s); }
    // THE admission sequence, in this order: a sharded param; a node fixed or freed since the factorisation; no retained factor; a
    // factor made from asymmetric information matrices
    int admit() {
        if (g_shard.find(param) != g_shard.end()) return refuse(ERR_UNSUPPORTED, "sharded params are not supported");
        auto it = g_ctx.find(param);
        if (it != g_ctx.end()) drop_factor_if_toggled(*it->second, g);
        if (it == g_ctx.end() || no_retained_factor(*it->second))
            return refuse(-1, "no retained factor (no successful solver call since the param was created or last failed)");
        if (it->second->fact_asym) return refuse(ERR_UNSUPPORTED, "the factorised graph holds factors with an asymmetric information matrix");
        cp = &*it->second;
        return 0;
    }
    Context &c() const { return *cp; }
    int N() const { return retained_N(*cp); }
    hipStream_t stream() { if (!s) s = take_stream(t_slot); return s; }
    __attribute__((format(printf, 3, 4))) int refuse(int code, const char *fmt, ...) const {
        va_list ap; va_start(ap, fmt);
        const int rc = refusev(code, who, fmt, ap);
        va_end(ap);
        return rc;
    }
    // second step, for the calls that read the graph's pack as the factorisation saw it (defined with the factor audit, solver_audit.inc.h)
    int linearisation(const char *what, GraphPack *&gpp, int &Fg);
};

// ------------------------------------------------------------------------------------------------------
// The view of the structure the retained factor lives in (Context::view): the plan of the last batch step (FACT_PLAN), or that plan with the
// incremental path's appended tail fronts and regenerated descriptors (FACT_EXTENDED: Context::inc -- descriptors, current parents, block
// maps and tail rows in the device arena d_i32, exactly what the factorisation read).  Validity, one rule for every reader: a view built
// for FACT_PLAN serves every later factorisation of that plan (upload_plan drops it, release_sel); an extended structure changes with
// every incremental step, so a FACT_EXTENDED view is rebuilt for every factorisation.  gen grows with every rebuild: the selected
// inversion's tables, the path solves' scratch maps and the tree solves' tables are kept against it.
static FactorView &factor_view(Context &c) {
    FactorView &V = c.view;
    if (V.kind == c.fact_kind && (V.kind == FACT_PLAN || V.serial == c.fact_serial)) return V;
    V.kind = FACT_NONE; V.on_device = false;
    const Plan &P = c.plan; const IncState &I = c.inc;
    const bool ext = c.fact_kind == FACT_EXTENDED;
    const int nF0 = P.nF, nFr = ext ? I.nF0 + (int)I.t_first.size() : P.nF, N = retained_N(c);
    if (ext && (I.nF0 != P.nF || I.Nb != P.N || (int)I.fd.size() < nFr || (int)I.parent.size() < nFr || (int)I.E.size() < nFr || (int)I.rel_begin.size() < nFr))
        fail(ERR_INTERNAL, "aprilsam_amd_marginals: incremental bookkeeping does not match the plan");
    std::vector<SelFront> &fr = V.fr;
    V.flops = 0;
    fr.assign((size_t)nFr, SelFront());
    V.depth.assign((size_t)nFr, 0);
    V.pool_end = 1;
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
        V.depth[t] = parent < 0 ? 0 : V.depth[parent] + 1;
        V.pool_end = std::max(V.pool_end, F.off + (long long)F.R * 3 * (nsb + nub));
        V.flops += 2.0 * F.u * F.u * F.s + (double)F.u * F.s * F.s + (double)F.s * F.s * F.s / 3.0;
    }
    // the fronts of every depth, root first and in ascending id: a front's parent is always one group earlier
    V.lev.assign(nFr ? (size_t)*std::max_element(V.depth.begin(), V.depth.end()) + 1 : 0, std::vector<int>());
    for (int t = 0; t < nFr; t++) V.lev[V.depth[t]].push_back(t);
    std::vector<int> &i32 = V.i32;
    i32.assign((size_t)2 * N, 0);                           // pos | pos_front
    for (int i = 0; i < N; i++) i32[i] = i < P.N ? P.pos[i] : i;                 // (a tail pose's position is its id)
    for (int t = 0; t < nF0; t++) for (int q = P.f_first[t]; q < P.f_first[t] + P.f_nsb[t]; q++) i32[N + q] = t;
    for (int q = P.N; q < N; q++) i32[N + q] = I.tf_of[q - P.N];
    V.N = N; V.serial = c.fact_serial; V.kind = c.fact_kind; V.gen++;
    return V;
}
// pos | pos_front of the current view on the device (pos_front = the pointer + N): THE device copy, uploaded when first asked for
static const int *view_pos(Context &c, hipStream_t s) {
    FactorView &V = factor_view(c);
    if (!V.on_device) {
        V.d_i32.need(std::max<size_t>(1, V.i32.size()));
        if (!V.i32.empty()) HIPCHECK(hipMemcpyAsync(V.d_i32.p, V.i32.data(), V.i32.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHECK(hipStreamSynchronize(s));                  // (a call that fails further on must not leave a copy in flight behind it)
        V.on_device = true;
    }
    return V.d_i32.p;
}
