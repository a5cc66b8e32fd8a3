// solver_pack.inc.h -- part of solver.hip.cpp (ONE translation unit: the kernels of kernels.hip.h are compiled once); included from there,
// inside namespace asam.  Contents: the packed graph: SoA mirrors of the caller's factor and node objects in pinned host memory and in HBM, one per april_graph_t.
// ------------------------------------------------------------------------------------------------------
// packed graph (SoA, host pinned + device) — one per april_graph_t pointer
// ------------------------------------------------------------------------------------------------------
static std::atomic<long long> g_pack_serial{ 0 };
static void forget_stream(hipStream_t s);      // solver_context.inc.h: no context may record an event on a stream that is about to be destroyed
// Streams are recycled per device slot.  On this runtime hipStreamCreateWithFlags takes 8 ms (a hardware queue) and hipStreamDestroy 2 ms
// (rocprofv3 --hip-trace, round 6): a graph's first solver call paid the former, its destruction the latter -- a program that builds a
// graph per solve (tools/soak_batch.py; a front end that re-creates its graph) paid both every time.  A released pack parks its idle
// stream; the next pack of that slot takes it.
constexpr int STREAM_POOL_MAX = 4;
static std::mutex g_stream_pool_mu;
static std::vector<hipStream_t> g_stream_pool[MAX_SLOTS];
static hipStream_t take_stream(int slot) {
    {
        std::lock_guard<std::mutex> lk(g_stream_pool_mu);
        auto &v = g_stream_pool[slot];
        if (!v.empty()) { hipStream_t s = v.back(); v.pop_back(); return s; }
    }
    hipStream_t s = nullptr;
    HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}
static void park_stream(int slot, hipStream_t s) {
    if (hipStreamSynchronize(s) == hipSuccess) {          // (idle, and healthy: a stream that reports an error is not handed on)
        std::lock_guard<std::mutex> lk(g_stream_pool_mu);
        auto &v = g_stream_pool[slot];
        if ((int)v.size() < STREAM_POOL_MAX) { v.push_back(s); return; }
    } else (void)hipGetLastError();
    (void)hipStreamDestroy(s);
}
// The device table of one factor family (max-mixture, robust, polar, dense Gaussian): columns of ints or doubles, one row per factor of the family, kept on
// the device append-only.  The host vectors and device buffers belong to the GraphPack, by name (kernels and the select_new_* rules read
// them); the table knows how they go up.  `gen` changes whenever the table's size or device addresses do: captured graphs are keyed by
// it (GraphPack::capture_key).
struct SideTable {
    // One column: `width` elements per row and `extra` behind the last row -- or, BY_COMP, per COMPONENT: the rows of such a column are the
    // table's prefix array (the max factors' z, W, c through mx_k).  Double columns are listed before int columns (staging alignment).
    // WRITTEN: the column a kernel writes (d_sel, d_rb_w: at most one) -- the host holds its values only for rows not yet uploaded.
    enum { WRITTEN = 1, BY_COMP = 2 };
    struct Col {
        std::vector<int> *hi = nullptr; DBuf<int> *di = nullptr; std::vector<double> *hd = nullptr; DBuf<double> *dd = nullptr; int width, extra; bool written, by_comp;
        template <class T> Col(std::vector<T> &h, DBuf<T> &d, int width = 1, int flags = 0, int extra = 0) : width(width), extra(extra), written(flags & WRITTEN), by_comp(flags & BY_COMP) {
            if constexpr (std::is_same<T, int>::value) { hi = &h; di = &d; } else { hd = &h; dd = &d; }
        }
        size_t esz() const { return hi ? 4 : 8; }
        const char *host() const { return hi ? (const char *)hi->data() : (const char *)hd->data(); }
        char *dev() const { return hi ? (char *)di->p : (char *)dd->p; }
        size_t cap() const { return hi ? di->cap : dd->cap; }
        void need(size_t n) const { if (hi) di->need(n); else dd->need(n); }
        void release() const { if (hi) di->release(); else dd->release(); }
        void clear() const { if (hi) hi->assign((size_t)extra, 0); else hd->clear(); }
    };
    const std::vector<int> &f;                      // the packed entry of each row: its size is the table's row count
    const std::vector<int> *prefix;                 // row -> first component (rows + 1 entries), or null: no column is by_comp
    std::vector<Col> cols;
    HBuf<double> stage;                             // pinned staging of every copy, packed as 8-byte words
    int on_device = 0; bool dirty = false; long long gen = 0;
    SideTable(const std::vector<int> &f, const std::vector<int> *prefix, std::vector<Col> cols) : f(f), prefix(prefix), cols(std::move(cols)) {}
    int rows() const { return (int)f.size(); }
    // elements of column c that rows [0, r) occupy (without `extra`)
    size_t upto(const Col &c, int r) const { return (size_t)c.width * (size_t)(c.by_comp ? (*prefix)[r] : r); }
    void clear() {
        if (rows() || on_device) gen++;             // (a pack that never held such factors keeps its captured graphs)
        for (const Col &c : cols) c.clear();
        on_device = 0; dirty = false;
    }
    const Col *written() const { for (const Col &c : cols) if (c.written) return &c; return nullptr; }
    // the device's values of the written column, rows [0, on_device), into out.  Through the pinned staging buffer: the stream is idle
    // before it is written (the caller has synchronised it)
    void read_back(hipStream_t s, void *out) {
        const Col *c = written();
        if (!c || on_device <= 0) return;
        const size_t bytes = c->esz() * (size_t)on_device;
        stage.need((bytes + 7) / 8);
        HIPCHECK(hipMemcpyAsync(stage.p, c->dev(), bytes, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        memcpy(out, stage.p, bytes);
    }
    // host -> device: what was appended since the last upload, everything after an edit (dirty) or a move.  The written column receives
    // the host's values of the appended rows only: the device's own of the older rows stay, and are carried across a move (read_back).
    // A buffer that is too small is allocated with head-room of half as much again and 64 rows: all of them move then
    void upload(hipStream_t s) {
        const int R = rows();
        if (R == 0 || (on_device == R && !dirty)) return;
        HIPCHECK(hipStreamSynchronize(s));          // (the pinned staging buffer is written below; this runs only when factors of the family were added or edited)
        bool fits = true;
        for (const Col &c : cols) fits = fits && upto(c, R) + c.extra <= c.cap();
        if (!fits) {
            if (const Col *c = written()) read_back(s, (void *)c->host());      // (the host's copy of these rows is stale or was never made)
            for (const Col &c : cols) { const size_t n = upto(c, R) / c.width; c.need((n + n / 2 + 64) * c.width + c.extra); }
            on_device = 0; dirty = true; gen++;
        }
        const int r0 = dirty ? 0 : on_device, w0 = std::min(on_device, R);
        auto first = [&](const Col &c) { return upto(c, c.written ? w0 : r0); };
        size_t bytes = 0;
        for (const Col &c : cols) bytes += c.esz() * (upto(c, R) + c.extra - first(c));
        stage.need((bytes + 7) / 8);
        char *st = (char *)stage.p;
        for (const Col &c : cols) {
            const size_t e0 = first(c), nb = c.esz() * (upto(c, R) + c.extra - e0);
            if (!nb) continue;
            memcpy(st, c.host() + c.esz() * e0, nb);
            HIPCHECK(hipMemcpyAsync(c.dev() + c.esz() * e0, st, nb, hipMemcpyHostToDevice, s));
            st += nb;
        }
        on_device = R; dirty = false;
    }
    void release() { for (const Col &c : cols) c.release(); stage.release(); }
};
// what a captured hipGraph of any kind depends on in the pack (GraphPack::capture_key), plus what that kind adds (`extra`, zero-filled)
struct CaptureKey {
    const void *state = nullptr; long long serial = 0, tables_gen = -1; std::array<size_t, 6> extra{};
    bool operator==(const CaptureKey &o) const { return state == o.state && serial == o.serial && tables_gen == o.tables_gen && extra == o.extra; }
};
struct GraphPack {
    int slot = 0;                      // device slot the pack's buffers and stream live on (solver.hip.cpp: SlotLock)
    const long long serial = ++g_pack_serial;      // captured hipGraphs are keyed by it: a pack freed and another allocated at the same addresses must not match
    int N = 0, F = 0;                  // packed counts (F: packed factor entries, see pack_factors)
    int Fg = 0;                        // graph factors packed (== F unless a factor has more than two nodes)
    std::vector<int> g2p, p2g;         // graph factor -> its first packed entry (size Fg + 1) / packed entry -> graph factor
    std::vector<unsigned> vslot;       // per packed entry of a host-evaluated factor: node slots (x << 8 | y; y = 0xff: unary) | carry bits << 16
    std::vector<const void *> fptr;    // factor object pointers already packed (cache validation), one per graph factor
    std::vector<int> pending;          // poses whose pinned state mirror is ahead of the device copy (written by apply_visits)
    HBuf<int> h_fa, h_fb;
    HBuf<double> h_z, h_W, h_state, h_lp, h_dx;
    DBuf<int> d_fa, d_fb;
    DBuf<double> d_z, d_W, d_state, d_lp, d_dx, d_chi2f, d_scalar;
    DBuf<double> d_lp_last; bool lp_last_valid = false;        // resident loops: the linearisation point of the LAST step enqueued (d_lp itself already holds the next one, UpdArgs::lp_next)
    int F_on_device = 0;               // factors already uploaded
    // whose linearisation the slots, d_lp and d_dx hold: the Context and fact_serial of the solver call that last linearised into the pack
    // and kept its factor (record_factor), at lin_content = content_version.  Every call that takes the pack to write into it clears the
    // stamp first (pack_for), so a step, LM or GNC run, or failed call of ANOTHER param on the graph leaves it not this param's (factor audit)
    const void *lin_ctx = nullptr; long long lin_serial = -1, lin_content = -1;
    int dirty_lo = 0, dirty_hi = 0;    // packed factors whose z / W changed since the last upload
    long long content_version = 0;     // bumped whenever z / W of a packed factor changed
    long long topo_version = 0;        // bumped whenever the packed endpoints (h_fa / h_fb, F) changed in any way: a pattern compared equal at (serial, topo_version) still is
    // factors whose information matrix is NOT symmetric as given (the reference's text loader fills W[1], W[2], W[5] and leaves W[3], W[6],
    // W[7] zero, examples/aprilsam_demo.c:73-75): the reference accumulates only blocks in the upper triangle of ITS elimination order with
    // W as given (aprilsam.c:171,520), so the off-diagonal block of such a factor depends on which endpoint it eliminates first
    // (solver_context.inc.h: orient_asymmetric)
    std::vector<unsigned char> asym; int n_asym = 0;
    void note_asym(int p, const double *w, bool device_factor) {
        const unsigned char a = device_factor && (w[1] != w[3] || w[2] != w[6] || w[5] != w[7]);
        if ((size_t)p >= asym.size()) asym.resize((size_t)p + 1, 0);
        n_asym += (int)a - (int)asym[p]; asym[p] = a;
    }
    std::vector<char> is_host;         // per factor: evaluated on the host through factor->eval
    std::vector<double> h_upt; DBuf<double> d_upt;   // unary factors: the state they were linearised at when they entered the system (3 per factor)
    int F_cap = 0;                     // device capacity (factors) of d_fa/d_fb/d_z/d_W/d_chi2f
    // factors of foreign types, evaluated on the host through factor->eval: indices, 33 doubles each
    // (Haa, Hab, Hbb, ga, gb), how many of them hold a current evaluation
    std::vector<int> host_idx; HBuf<double> h_hostH; DBuf<double> d_hostH; DBuf<int> d_host_idx; int host_evaluated = 0;
    // max-mixture factors: per max factor m its packed entry mx_f[m] and components [mx_k[m], mx_k[m + 1]); per
    // component z (3), W (9), c = -2 logw - ln det W and logw as given (content check); mx_sel: the selection made on the host (incremental
    // steps; -1: none yet) -- d_sel, written by k_select_mixture, holds the selection of each factor's most recent linearisation.  mx_of: per
    // graph factor its m or -1
    std::vector<int> mx_f, mx_k{ 0 }, mx_sel, mx_of; std::vector<double> mx_z, mx_W, mx_c, mx_logw;
    DBuf<int> d_mx_f, d_mx_k, d_sel; DBuf<double> d_mx_z, d_mx_W, d_mx_c;
    SideTable mx{ mx_f, &mx_k, { { mx_z, d_mx_z, 3, SideTable::BY_COMP }, { mx_W, d_mx_W, 9, SideTable::BY_COMP }, { mx_c, d_mx_c, 1, SideTable::BY_COMP }, { mx_f, d_mx_f }, { mx_k, d_mx_k, 1, 0, 1 }, { mx_sel, d_sel, 1, SideTable::WRITTEN } } };
    int n_max() const { return (int)mx_f.size(); }
    void mx_clear() { mx.clear(); mx_of.clear(); mx_logw.clear(); }
    // robust factors: per robust factor q its packed entry rb_f[q], kind rb_kind[q], scale rb_c[q] and unweighted
    // information matrix rb_W0[9q] (the slot of h_W / d_W holds W_eff = w W0 once a linearisation weighted it); rb_w: the host's weight
    // (incremental steps; -1: none yet) -- d_rb_w, written by k_robust_weight, holds the weight of each factor's most recent linearisation.
    // rb_of: per graph factor its q or -1
    std::vector<int> rb_f, rb_kind, rb_of; std::vector<double> rb_c, rb_W0, rb_w;
    DBuf<int> d_rb_f, d_rb_kind; DBuf<double> d_rb_c, d_rb_W0, d_rb_w;
    SideTable rb{ rb_f, nullptr, { { rb_W0, d_rb_W0, 9 }, { rb_c, d_rb_c }, { rb_w, d_rb_w, 1, SideTable::WRITTEN }, { rb_f, d_rb_f }, { rb_kind, d_rb_kind } } };
    int n_robust() const { return (int)rb_f.size(); }
    void rb_clear() { rb.clear(); rb_of.clear(); }
    // polar factors (polar.hip.h): per polar factor p its packed entry pl_f[p], kind pl_kind[p], measurement pl_z[2p] and
    // information matrix pl_W[4p] (the slot of h_z / h_W holds a null placeholder until k_polar_slot or select_new_polar writes z_eff / W_eff).
    // pl_of: per graph factor its p or -1
    std::vector<int> pl_f, pl_kind, pl_of; std::vector<double> pl_z, pl_W;
    DBuf<int> d_pl_f, d_pl_kind; DBuf<double> d_pl_z, d_pl_W;
    SideTable pl{ pl_f, nullptr, { { pl_z, d_pl_z, 2 }, { pl_W, d_pl_W, 4 }, { pl_f, d_pl_f }, { pl_kind, d_pl_kind } } };
    int n_polar() const { return (int)pl_f.size(); }
    void pl_clear() { pl.clear(); pl_of.clear(); }
    // dense Gaussian factors (gaussian.hip.h): per Gaussian factor q its FIRST packed entry gs_f[q] (the entries of the
    // clique of its node pairs follow), its node count gs_k[q] and, in fixed-width rows padded to GS_MAX nodes, the node ids gs_node[11q],
    // xbar gs_xbar[33q], eta gs_eta[33q], Lambda gs_L[1089q] (3k x 3k, row stride 3k) and the chi^2 constant gs_c0[q].  The entries' slots
    // of h_z / h_W hold null factors for good.  gs_of: per graph factor its q or -1
    std::vector<int> gs_f, gs_k, gs_node, gs_of; std::vector<double> gs_xbar, gs_eta, gs_L, gs_c0;
    DBuf<int> d_gs_f, d_gs_k, d_gs_node; DBuf<double> d_gs_xbar, d_gs_eta, d_gs_L, d_gs_c0;
    SideTable gs{ gs_f, nullptr, { { gs_xbar, d_gs_xbar, GS_ROWS }, { gs_eta, d_gs_eta, GS_ROWS }, { gs_L, d_gs_L, GS_LSZ }, { gs_c0, d_gs_c0 }, { gs_f, d_gs_f }, { gs_k, d_gs_k }, { gs_node, d_gs_node, GS_MAX } } };
    int n_gaussian() const { return (int)gs_f.size(); }
    void gs_clear() { gs.clear(); gs_of.clear(); }
    GaussTab gauss_tab() const { return GaussTab{ n_gaussian(), d_gs_f.p, d_gs_k.p, d_gs_node.p, d_gs_xbar.p, d_gs_eta.p, d_gs_L.p, d_gs_c0.p }; }
    // fixed nodes (fixed.hip.h): fx_nodes: the ids of the nodes held constant, ascending, as the last call's walk over
    // the node objects found them (sync_fixed); fx_rec: one record per packed entry with a fixed endpoint (.x the entry, .y the FX_* bits of
    // the slots k_fix_mask zeroes), built from the PACKED entries -- the pairs of a host-evaluated clique included -- at fx_topo =
    // topo_version.  fx_gen changes whenever the set or the records do: captured graphs are keyed by it, and d_lambda's host cache
    std::vector<int> fx_nodes; std::vector<int2> fx_rec; long long fx_topo = -1;
    DBuf<int> d_fx_nodes; DBuf<int2> d_fx_rec;
    bool fx_dirty = false; long long fx_gen = 0;
    int n_fixed() const { return (int)fx_nodes.size(); }
    // What every captured graph reads of the pack: the device arrays (d_state stands for all that grow with the nodes), this pack and no
    // other at the same addresses, and every side table where it lay at the capture.  Each generation only grows, so their sum changes
    // exactly when one of them does: a new table-keeping family adds its generation to this sum and is keyed everywhere
    CaptureKey capture_key(std::array<size_t, 6> extra = {}) const { return CaptureKey{ d_state.p, serial, mx.gen + rb.gen + pl.gen + gs.gen + fx_gen, extra }; }
    // GNC candidates (gnc.hip.h): a table that exists on the device for the length of ONE aprilsam_amd_optimize_gnc
    // call -- gc_n > 0 only inside it.  d_gc_f / d_gc_W0 / d_gc_w: packed entry, plain W and last weight per candidate, d_gc_par: loss, c
    // and mu; d_gc_out / gc_stage: results and their pinned staging.  gc_gen changes with every run: captured LM iterations are keyed by it
    DBuf<int> d_gc_f; DBuf<double> d_gc_W0, d_gc_w, d_gc_out; DBuf<GncPar> d_gc_par; HBuf<double> gc_stage;
    int gc_n = 0; long long gc_gen = 0;
    hipStream_t stream = nullptr;
    HBuf<double> h_scalar;
    // incremental steps: the pinned mirrors h_state / h_lp and the device arrays d_state / d_lp hold the same values (mirror_sync),
    // so a step only has to patch the poses whose host objects differ from the mirror (pack_states_diff); the step's new
    // states go to h_out (pinned), not into the mirror
    HBuf<double> h_out; bool mirror_sync = false; std::vector<int> changed; const double *new_states = nullptr;
    void release() {
        h_out.release(); mirror_sync = false;
        h_fa.release(); h_fb.release(); h_z.release(); h_W.release(); h_state.release(); h_lp.release(); h_dx.release();
        d_fa.release(); d_fb.release(); d_z.release(); d_W.release(); d_state.release(); d_lp.release(); d_lp_last.release(); d_dx.release();
        d_chi2f.release(); d_scalar.release(); h_scalar.release(); h_hostH.release(); d_hostH.release(); d_host_idx.release(); d_upt.release();
        mx.release(); mx_clear();
        rb.release(); rb_clear();
        pl.release(); pl_clear();
        gs.release(); gs_clear();
        d_fx_nodes.release(); d_fx_rec.release(); fx_nodes.clear(); fx_rec.clear(); fx_topo = -1; fx_dirty = false;
        d_gc_f.release(); d_gc_W0.release(); d_gc_w.release(); d_gc_out.release(); d_gc_par.release(); gc_stage.release(); gc_n = 0;
        if (stream) { forget_stream(stream); park_stream(slot, stream); }
        stream = nullptr;
    }
};

static Registry<GraphPack> g_packs;

static int slot_of_graph(const void *g) {
    int slot = -1;
    g_packs.with(g, [&](GraphPack &gp) { slot = gp.slot; });
    return slot;
}
// the pack of a graph, on the slot of the call in progress (a pack left behind on another slot by an earlier call moves: dropped there,
// rebuilt here -- one graph is driven from one slot at a time)
static GraphPack &pack_for(const april_graph_t *g, bool keep_lin = false) {
    auto it = g_packs.find(g);
    if (it != g_packs.end() && it->second->slot != t_slot) {
        // The pack is released under the OLD slot's lock as well, so that no call on that slot is inside it (april_graph_chi2 or a destroy
        // found by the graph alone).  That lock is tried, not waited for without bound: this thread holds its own slot, and two threads
        // moving graphs in opposite directions must not wait for each other forever -- normally the other slot is busy with ANOTHER
        // graph's call and frees up within that call's time
        const int os = it->second->slot;
        std::unique_lock<std::mutex> old_slot(g_slot_mu[os], std::try_to_lock);
        for (const auto t0 = std::chrono::steady_clock::now(); !old_slot.owns_lock(); (void)old_slot.try_lock()) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
                fail(ERR_UNSUPPORTED, "graph %p was last solved on device slot %d, which other threads kept busy for 10 s: one graph is driven from one slot at a "
                     "time (the call on slot %d did nothing)", (const void *)g, os, t_slot);
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        it = g_packs.find(g);
        if (it != g_packs.end() && it->second->slot != t_slot) { it->second->release(); g_packs.erase(it); it = g_packs.end(); }
    }
    if (it == g_packs.end()) {
        auto p = std::make_unique<GraphPack>();
        p->slot = t_slot;
        p->stream = take_stream(t_slot);
        it = g_packs.emplace(g, std::move(p)).first;
    }
    if (!keep_lin) it->second->lin_ctx = nullptr;      // (keep_lin: a call that linearises nothing -- april_graph_chi2)
    return *it->second;
}
void drop_graph_pack(const april_graph_t *g) {
    SlotLock lk(nullptr, g);
    auto it = g_packs.find(g);
    if (it != g_packs.end()) { it->second->release(); g_packs.erase(it); }
}

static inline int zsize(const zarray_t *z) { return z ? z->size : 0; }

// (re)pack the factors: ids, z, W into the pinned SoA mirror.  The reference re-reads every factor object on every call
// (aprilsam.c:152-190, april_graph.c:79-98), so by default every already-packed factor is compared with the mirror
// (nodes, z, W: 104 bytes) and only what changed is copied and uploaded again; a changed endpoint or factor kind
// restarts the pack.  Option trust_factor_cache = 1 skips the comparison for factors whose object pointer is unchanged
// (z / W of a packed factor are then treated as immutable).
//
// PACKED factors are what everything below this function sees: one entry per graph factor with one or two nodes, and for a
// factor with k >= 3 nodes (foreign types only, evaluated through their own eval(): the reference's assembly loops are
// generic over factor->nnodes, aprilsam.c:159-192) one entry per PAIR of its nodes, k (k - 1) / 2 of them -- the pair (i, j)
// carries the off-diagonal block J_i^T W J_j; the diagonal block and the right-hand-side segment of node i ride on the
// first pair that contains i.  A clique of binary entries is exactly the structure such a factor has in the normal
// equations, so ordering, symbolic analysis and kernels need not know.  gp.F counts packed entries, gp.Fg graph factors
// (param->factor_num, aprilsam.c:283-288); g2p / p2g translate.
static void pack_factors(GraphPack &gp, const april_graph_t *g, bool validate_old = true) {
    const bool trust = g_opt.trust_factor_cache || !validate_old;      // (incremental calls never re-read old factors, aprilsam.c:508-511)
    const int Fg = zsize(g->factors);
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    const int N = zsize(g->nodes);
    int from = gp.Fg;
    bool valid = from <= Fg && (int)gp.fptr.size() == from && (int)gp.g2p.size() == from + 1;
    // (incremental calls only ever look at the factors added since the previous call, aprilsam.c:508-511: first and last packed pointer
    // as a sanity check instead of all of them -- the comparison of 5 000 pointers was a microsecond of every step)
    if (valid && trust) valid = from == 0 || (validate_old ? memcmp(gp.fptr.data(), fs, sizeof(void *) * from) == 0 : (gp.fptr[0] == fs[0] && gp.fptr[from - 1] == fs[from - 1]));
    auto restart = [&]() { gp.topo_version++; from = 0; gp.F = 0; gp.F_on_device = 0; gp.host_idx.clear(); gp.host_evaluated = 0; gp.is_host.clear(); gp.p2g.clear(); gp.vslot.clear(); gp.g2p.assign(1, 0); gp.asym.clear(); gp.n_asym = 0; gp.mx_clear(); gp.rb_clear(); gp.pl_clear(); gp.gs_clear(); };
    if (!valid) restart();
    // one graph factor -> its packed entries (a, b, host flag, node slots of a host pair, what the pair carries)
    struct Ent { int a, b; bool host; unsigned short slots; unsigned char carry; };
    Ent ents[64]; int ne = 0; bool is_max = false, is_rb = false, is_pl = false, is_gs = false; int rb_kind = 0, pl_kind = 0, gs_k = 0; double rb_c = 0, gs_c0 = 0;
    auto classify = [&](const april_graph_factor_t *f, int i) {
        ne = 0; is_max = false; is_rb = false; is_pl = false; is_gs = false;
        if (is_native_max(f)) {        // (before anything reads u.common: u.max aliases it)
            char why[192];
            if (f->nnodes != 2 || !max_check(f, why, sizeof why)) fail(ERR_UNSUPPORTED, "factor %d: max factor: %s", i, f->nnodes != 2 ? "not binary" : why);
            ents[ne++] = Ent{ f->nodes[0], f->nodes[1], false, 0, 3 }; is_max = true;
        } else if (f->type == APRIL_GRAPH_FACTOR_XYT_TYPE && f->nnodes == 2) { ents[ne++] = Ent{ f->nodes[0], f->nodes[1], false, 0, 3 }; is_rb = robust_of(f, &rb_kind, &rb_c); }
        else if (f->type == APRIL_GRAPH_FACTOR_XYTPOS_TYPE && f->nnodes == 1) { ents[ne++] = Ent{ f->nodes[0], -1, false, 0, 3 }; is_rb = robust_of(f, &rb_kind, &rb_c); }
        else if (!g_opt.polar_on_host && polar_of(f, &pl_kind)) {      // this library's range / bearing / range-bearing factor
            const int m = polar_rows(pl_kind);
            bool ok = (int)f->u.common.W->nrows == m && (int)f->u.common.W->ncols == m && polar_spd(pl_kind, f->u.common.W->data);
            for (int k = 0; k < m && ok; k++) ok = std::isfinite(f->u.common.z[k]);     // (the constructor checked both; the caller may have edited them since)
            if (!ok) fail(ERR_UNSUPPORTED, "factor %d: a polar factor's z must be finite and its W finite, symmetric and positive definite (DESIGN.md section 19)", i);
            ents[ne++] = Ent{ f->nodes[0], f->nodes[1], false, 0, 3 }; is_pl = true;
        }
        else if (bool gs_ok = false; !g_opt.gaussian_on_host && gaussian_ever() && gaussian_of(f, &gs_k, &gs_c0, &gs_ok)) {      // this library's dense Gaussian factor
            bool ok = gs_ok && gs_k >= 1 && gs_k <= GS_MAX;
            for (int r = 0; r < 3 * gs_k && ok; r++) ok = std::isfinite(f->u.common.z[r]);      // (the constructor checked all of it; the caller may have edited xbar, eta or Lambda since)
            if (!ok) fail(ERR_UNSUPPORTED, "factor %d: a Gaussian factor's xbar and eta must be finite and its Lambda finite, symmetric and positive semi-definite (DESIGN.md section 24)", i);
            // the clique of its node pairs in the host clique's order, slots and carry bits -- device entries: their slots of z / W are null
            // factors, k_gaussian_slot writes their contributions
            if (gs_k == 1) ents[ne++] = Ent{ f->nodes[0], -1, false, 0xff, 3 };
            for (int x = 0; x < gs_k; x++)
                for (int y = x + 1; y < gs_k; y++) {
                    const unsigned char carry = (unsigned char)(((x == 0 && y == 1) ? 1 : 0) | ((x == 0) ? 2 : 0));
                    ents[ne++] = Ent{ f->nodes[x], f->nodes[y], false, (unsigned short)((x << 8) | y), carry };
                }
            is_gs = true;
        }
        else if ((f->nnodes == 1 || f->nnodes == 2) && f->eval)       // any other type: the factor's own eval(), on the host
            ents[ne++] = Ent{ f->nodes[0], f->nnodes == 2 ? f->nodes[1] : -1, true, (unsigned short)(f->nnodes == 2 ? 1 : 0xff), 3 };
        else if (f->nnodes >= 3 && f->nnodes <= 11 && f->eval) {      // a clique of pairs (see above); 11 nodes = 55 pairs
            for (int x = 0; x < f->nnodes; x++)
                for (int y = x + 1; y < f->nnodes; y++) {
                    // node x's diagonal block / rhs on its first pair: (0, 1) for x = 0 and x = 1, (0, x) beyond
                    const unsigned char carry = (unsigned char)(((x == 0 && y == 1) ? 1 : 0) | ((x == 0) ? 2 : 0));
                    ents[ne++] = Ent{ f->nodes[x], f->nodes[y], true, (unsigned short)((x << 8) | y), carry };
                }
        } else {
            fail(ERR_UNSUPPORTED, "factor %d has type %d / %d nodes; factors of foreign types are supported with 1 to 11 nodes and an "
                                  "eval() function pointer (aprilsam.h:110-122)", i, f->type, f->nnodes);
        }
        if (is_rb && !robust_spd(f->u.common.W->data))       // (set_robust checked it; the caller may have edited W since)
            fail(ERR_UNSUPPORTED, "factor %d: a robust factor's W must be symmetric positive definite (DESIGN.md section 15)", i);
        for (int e = 0; e < ne; e++) {
            // -1 in `b` is the internal marker of a unary entry: a graph factor with two or more nodes must name real nodes on both sides
            // (a negative second endpoint used to pass as "unary" with its node slots still naming the missing node)
            if (ents[e].a < 0 || ents[e].a >= N || ents[e].b >= N || (f->nnodes >= 2 && ents[e].b < 0))
                fail(ERR_BAD_GRAPH, "factor %d references node %d / %d of %d", i, ents[e].a, ents[e].b, N);
            if (ents[e].a == ents[e].b) fail(ERR_BAD_GRAPH, "factor %d connects node %d to itself", i, ents[e].a);
        }
    };
    if (from > 0 && !trust) {
        // content check of the packed prefix; dirty range [lo, hi) is uploaded again by upload_factors
        int lo = gp.F, hi = 0;
        bool changed = false;
        for (int i = 0; i < from; i++) {
            if (i + 8 < from) __builtin_prefetch(fs[i + 8]);
            const april_graph_factor_t *f = fs[i];
            classify(f, i);
            const int p0 = gp.g2p[i];
            if (gp.g2p[i + 1] - p0 != ne) { changed = true; break; }
            for (int e = 0; e < ne && !changed; e++)
                changed = ents[e].a != gp.h_fa.p[p0 + e] || ents[e].b != gp.h_fb.p[p0 + e] || ents[e].host != (bool)gp.is_host[p0 + e];
            if (!changed) changed = is_max != (gp.mx_of[i] >= 0) || (is_max && gp.mx_k[gp.mx_of[i] + 1] - gp.mx_k[gp.mx_of[i]] != f->u.max.nfactors);
            if (!changed) changed = is_rb != (i < (int)gp.rb_of.size() && gp.rb_of[i] >= 0);      // (a loss gained or lost: the table is packed again)
            if (!changed) changed = is_pl != (i < (int)gp.pl_of.size() && gp.pl_of[i] >= 0) || (is_pl && gp.pl_kind[gp.pl_of[i]] != pl_kind);
            if (!changed) changed = is_gs != (i < (int)gp.gs_of.size() && gp.gs_of[i] >= 0) || (is_gs && gp.gs_k[gp.gs_of[i]] != gs_k);
            if (changed) break;
            gp.fptr[i] = f;
            if (ents[0].host) continue;
            if (is_gs) {               // the slots hold null factors: the object against the table
                const int q = gp.gs_of[i], n = 3 * gs_k;
                double *tx = gp.gs_xbar.data() + (size_t)GS_ROWS * q, *te = gp.gs_eta.data() + (size_t)GS_ROWS * q, *tL = gp.gs_L.data() + (size_t)GS_LSZ * q;
                if (memcmp(tx, f->u.common.z, (size_t)8 * n) != 0 || memcmp(te, f->u.common.z + n, (size_t)8 * n) != 0 ||
                    memcmp(tL, f->u.common.W->data, (size_t)8 * n * n) != 0) {
                    memcpy(tx, f->u.common.z, (size_t)8 * n); memcpy(te, f->u.common.z + n, (size_t)8 * n); memcpy(tL, f->u.common.W->data, (size_t)8 * n * n);
                    gp.gs_c0[q] = gs_c0;
                    gp.gs.dirty = true; lo = std::min(lo, p0); hi = std::max(hi, p0 + 1);
                }
                continue;
            }
            if (is_max) {              // the components against the table: an edited one is copied and the table uploaded again
                const int m = gp.mx_of[i];
                bool edit = false;
                for (int k = gp.mx_k[m], j = 0; k < gp.mx_k[m + 1]; k++, j++) {
                    const april_graph_factor_t *cf = f->u.max.factors[j];
                    double *zp = gp.mx_z.data() + (size_t)3 * k, *Wp = gp.mx_W.data() + (size_t)9 * k;
                    if (memcmp(zp, cf->u.common.z, 24) != 0 || memcmp(Wp, cf->u.common.W->data, 72) != 0 || memcmp(&gp.mx_logw[k], &f->u.max.logw[j], 8) != 0) {
                        memcpy(zp, cf->u.common.z, 24); memcpy(Wp, cf->u.common.W->data, 72);
                        gp.mx_logw[k] = f->u.max.logw[j]; gp.mx_c[k] = max_const(f, j);
                        edit = true;
                    }
                }
                if (edit) { gp.mx.dirty = true; lo = std::min(lo, p0); hi = std::max(hi, p0 + 1); }
                continue;
            }
            if (is_pl) {               // the slot holds z_eff / W_eff: the object against the table
                const int q = gp.pl_of[i], m = polar_rows(pl_kind);
                double *tz = gp.pl_z.data() + (size_t)2 * q, *tW = gp.pl_W.data() + (size_t)4 * q;
                if (memcmp(tz, f->u.common.z, (size_t)8 * m) != 0 || memcmp(tW, f->u.common.W->data, (size_t)8 * m * m) != 0) {
                    memcpy(tz, f->u.common.z, (size_t)8 * m); memcpy(tW, f->u.common.W->data, (size_t)8 * m * m);
                    gp.pl.dirty = true; lo = std::min(lo, p0); hi = std::max(hi, p0 + 1);
                }
                continue;
            }
            double *zp = gp.h_z.p + (size_t)3 * p0, *Wp = gp.h_W.p + (size_t)9 * p0;
            if (is_rb) {               // the slot holds W_eff: z and W against the table's W0, kind and c against the table
                const int q = gp.rb_of[i];
                double *W0 = gp.rb_W0.data() + (size_t)9 * q;
                if (memcmp(zp, f->u.common.z, 24) != 0 || memcmp(W0, f->u.common.W->data, 72) != 0 || gp.rb_kind[q] != rb_kind || memcmp(&gp.rb_c[q], &rb_c, 8) != 0) {
                    memcpy(zp, f->u.common.z, 24); memcpy(W0, f->u.common.W->data, 72); memcpy(Wp, W0, 72);
                    gp.rb_kind[q] = rb_kind; gp.rb_c[q] = rb_c;
                    gp.rb.dirty = true; lo = std::min(lo, p0); hi = std::max(hi, p0 + 1);
                }
                continue;
            }
            if (memcmp(zp, f->u.common.z, 24) != 0 || memcmp(Wp, f->u.common.W->data, 72) != 0) {
                memcpy(zp, f->u.common.z, 24); memcpy(Wp, f->u.common.W->data, 72);
                gp.note_asym(p0, Wp, true);
                lo = std::min(lo, p0); hi = std::max(hi, p0 + 1);
            }
        }
        if (changed) restart();
        else if (hi > lo) {
            if (gp.dirty_hi > gp.dirty_lo) { gp.dirty_lo = std::min(gp.dirty_lo, lo); gp.dirty_hi = std::max(gp.dirty_hi, hi); }
            else { gp.dirty_lo = lo; gp.dirty_hi = hi; }
            gp.content_version++;
        }
    }
    gp.fptr.resize(Fg); gp.g2p.resize((size_t)Fg + 1); gp.mx_of.resize(Fg, -1); gp.rb_of.resize(Fg, -1); gp.pl_of.resize(Fg, -1); gp.gs_of.resize(Fg, -1);
    int F = gp.g2p[from];
    {   // the pinned mirrors are sized ONCE for everything this call appends (a pinned reallocation costs a quarter of a millisecond)
        size_t total = (size_t)F;
        for (int i = from; i < Fg; i++) {
            // arity is checked BEFORE anything is sized from it: a foreign factor with a garbage nnodes must end in ERR_UNSUPPORTED
            // (classify() below says so), not in a pinned allocation of k (k - 1) / 2 entries
            const int k = fs[i]->nnodes;
            total += (k >= 3 && k <= 11) ? (size_t)k * (k - 1) / 2 : 1;
        }
        gp.h_fa.need(total, true); gp.h_fb.need(total, true); gp.h_z.need(3 * total, true); gp.h_W.need(9 * total, true);
        gp.is_host.resize(total, 0); gp.p2g.resize(total); gp.vslot.resize(total);
    }
    if (from < Fg || gp.F != F) gp.topo_version++;
    for (int i = from; i < Fg; i++) {
        const april_graph_factor_t *f = fs[i];
        gp.fptr[i] = f;
        classify(f, i);
        for (int e = 0; e < ne; e++, F++) {
            gp.h_fa.p[F] = ents[e].a; gp.h_fb.p[F] = ents[e].b; gp.is_host[F] = ents[e].host; gp.p2g[F] = i;
            gp.vslot[F] = (unsigned)ents[e].slots | ((unsigned)ents[e].carry << 16);
            if (ents[e].host) {          // the device kernels see a null factor (W = 0) in its place; k_scatter_host fills its slots
                memset(gp.h_z.p + (size_t)3 * F, 0, 24); memset(gp.h_W.p + (size_t)9 * F, 0, 72);
                gp.note_asym(F, gp.h_W.p + (size_t)9 * F, false);
                gp.host_idx.push_back(F);
            } else if (is_gs) {        // every entry of the clique holds a null factor (symmetric) for good; the factor's row goes in with its first entry
                memset(gp.h_z.p + (size_t)3 * F, 0, 24); memset(gp.h_W.p + (size_t)9 * F, 0, 72);
                gp.note_asym(F, gp.h_W.p + (size_t)9 * F, true);
                if (e > 0) continue;
                const int n = 3 * gs_k;
                gp.gs_of[i] = gp.n_gaussian(); gp.gs_f.push_back(F); gp.gs_k.push_back(gs_k); gp.gs_c0.push_back(gs_c0);
                const size_t q = gp.gs_k.size() - 1;
                gp.gs_node.resize((q + 1) * GS_MAX, 0); gp.gs_xbar.resize((q + 1) * GS_ROWS, 0.0); gp.gs_eta.resize((q + 1) * GS_ROWS, 0.0); gp.gs_L.resize((q + 1) * GS_LSZ, 0.0);
                memcpy(&gp.gs_node[q * GS_MAX], f->nodes, (size_t)4 * gs_k);
                memcpy(&gp.gs_xbar[q * GS_ROWS], f->u.common.z, (size_t)8 * n); memcpy(&gp.gs_eta[q * GS_ROWS], f->u.common.z + n, (size_t)8 * n);
                memcpy(&gp.gs_L[q * GS_LSZ], f->u.common.W->data, (size_t)8 * n * n);
                gp.gs.gen++;
            } else if (is_max) {       // the slot holds component 0 until a selection writes it (k_select_mixture, select_new_max)
                const april_graph_factor_t *c0 = f->u.max.factors[0];
                memcpy(gp.h_z.p + (size_t)3 * F, c0->u.common.z, 24);
                memcpy(gp.h_W.p + (size_t)9 * F, c0->u.common.W->data, 72);
                gp.note_asym(F, gp.h_W.p + (size_t)9 * F, true);
                gp.mx_of[i] = gp.n_max(); gp.mx_f.push_back(F); gp.mx_sel.push_back(-1);
                for (int j = 0; j < f->u.max.nfactors; j++) {
                    const april_graph_factor_t *cf = f->u.max.factors[j];
                    gp.mx_z.insert(gp.mx_z.end(), cf->u.common.z, cf->u.common.z + 3);
                    gp.mx_W.insert(gp.mx_W.end(), cf->u.common.W->data, cf->u.common.W->data + 9);
                    gp.mx_c.push_back(max_const(f, j)); gp.mx_logw.push_back(f->u.max.logw[j]);
                }
                gp.mx_k.push_back((int)gp.mx_c.size());
                gp.mx.gen++;
            } else if (is_pl) {        // the slot holds a null factor (symmetric) until k_polar_slot / select_new_polar writes z_eff / W_eff
                memset(gp.h_z.p + (size_t)3 * F, 0, 24); memset(gp.h_W.p + (size_t)9 * F, 0, 72);
                gp.note_asym(F, gp.h_W.p + (size_t)9 * F, true);
                const int m = polar_rows(pl_kind);
                double tz[2] = { 0, 0 }, tW[4] = { 0, 0, 0, 0 };
                memcpy(tz, f->u.common.z, (size_t)8 * m); memcpy(tW, f->u.common.W->data, (size_t)8 * m * m);
                gp.pl_of[i] = gp.n_polar(); gp.pl_f.push_back(F); gp.pl_kind.push_back(pl_kind);
                gp.pl_z.insert(gp.pl_z.end(), tz, tz + 2); gp.pl_W.insert(gp.pl_W.end(), tW, tW + 4);
                gp.pl.gen++;
            } else {
                memcpy(gp.h_z.p + (size_t)3 * F, f->u.common.z, 24);
                memcpy(gp.h_W.p + (size_t)9 * F, f->u.common.W->data, 72);
                gp.note_asym(F, gp.h_W.p + (size_t)9 * F, true);
                if (is_rb) {           // the slot holds W0 until a weighting writes W_eff (k_robust_weight, select_new_robust)
                    gp.rb_of[i] = gp.n_robust(); gp.rb_f.push_back(F); gp.rb_kind.push_back(rb_kind); gp.rb_c.push_back(rb_c); gp.rb_w.push_back(-1.0);
                    gp.rb_W0.insert(gp.rb_W0.end(), f->u.common.W->data, f->u.common.W->data + 9);
                    gp.rb.gen++;
                }
            }
        }
        gp.g2p[i + 1] = F;
    }
    gp.F = F; gp.Fg = Fg;
}
// incremental steps: the max factors packed at or after entry f_from are selected on the host at the l_point mirror (max_select, the rule
// k_select_mixture applies) and their slots of h_z / h_W take the winner -- the fast path uploads and linearises them as plain xyt factors
static void select_new_max(GraphPack &gp, const april_graph_t *g, int f_from) {
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    for (int m = gp.n_max() - 1; m >= 0 && gp.mx_f[m] >= f_from; m--) {
        const int p = gp.mx_f[m];
        const april_graph_factor_t *f = fs[gp.p2g[p]];
        const int k = max_select(f, gp.h_lp.p + (size_t)3 * gp.h_fa.p[p], gp.h_lp.p + (size_t)3 * gp.h_fb.p[p]);
        gp.mx_sel[m] = k;
        memcpy(gp.h_z.p + (size_t)3 * p, &gp.mx_z[(size_t)3 * (gp.mx_k[m] + k)], 24);
        memcpy(gp.h_W.p + (size_t)9 * p, &gp.mx_W[(size_t)9 * (gp.mx_k[m] + k)], 72);
    }
}
// incremental steps: the robust factors packed at or after entry f_from are weighted on the host (robust_host_s + robust_weight, the rule
// k_robust_weight applies) at the point the fast path linearises them -- the l_point mirror (xyt) or the state mirror (xytpos, as
// record_unary_points) -- and their slots of h_W take W_eff = w W0
static void select_new_robust(GraphPack &gp, int f_from) {
    for (int q = gp.n_robust() - 1; q >= 0 && gp.rb_f[q] >= f_from; q--) {
        const int p = gp.rb_f[q], a = gp.h_fa.p[p], b = gp.h_fb.p[p];
        const double *W0 = gp.rb_W0.data() + (size_t)9 * q;
        const double s = robust_host_s(gp.h_z.p + (size_t)3 * p, W0, b >= 0 ? gp.h_lp.p + (size_t)3 * a : gp.h_state.p + (size_t)3 * a,
                                       b >= 0 ? gp.h_lp.p + (size_t)3 * b : nullptr);
        const double w = robust_weight(gp.rb_kind[q], gp.rb_c[q], s);
        gp.rb_w[q] = w;
        for (int k = 0; k < 9; k++) gp.h_W.p[(size_t)9 * p + k] = w * W0[k];
    }
}
// incremental steps: the slots of the polar factors packed at or after entry f_from are written on the host (polar.h, the formulas
// k_polar_slot applies) at the l_point mirror -- the fast path uploads and linearises them as plain xyt factors
static void select_new_polar(GraphPack &gp, int f_from) {
    for (int q = gp.n_polar() - 1; q >= 0 && gp.pl_f[q] >= f_from; q--) {
        const int p = gp.pl_f[q], a = gp.h_fa.p[p], b = gp.h_fb.p[p];
        polar_host_slot(gp.pl_kind[q], gp.pl_z.data() + (size_t)2 * q, gp.pl_W.data() + (size_t)4 * q, gp.h_lp.p + (size_t)3 * a, gp.h_lp.p + (size_t)3 * b,
                        gp.h_z.p + (size_t)3 * p, gp.h_W.p + (size_t)9 * p);
    }
}
// ---- fixed nodes -------------------------------------------------------------------------------------
// the first fixed node of a graph, -1 when it has none (a process that never fixed a node does not walk)
static int first_fixed(const april_graph_t *g) {
    if (!g || !fixed_ever()) return -1;
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0, N = zsize(g->nodes); i < N; i++) if (node_fixed(ns[i])) return i;
    return -1;
}
static void scan_fixed(const april_graph_t *g, std::vector<int> &out) {
    out.clear();
    if (!g || !fixed_ever()) return;
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0, N = zsize(g->nodes); i < N; i++) if (node_fixed(ns[i])) out.push_back(i);
}
// The entry points that do not take fixed nodes: 0, or -12 with a message that names the first fixed node.  Nothing was read or written
// before; the param keeps its plan and factor (the refusal is recorded, not thrown).
static int refuse_fixed(const char *who, const april_graph_t *g) {
    const int i = first_fixed(g);
    if (i < 0) return 0;
    char msg[320];
    snprintf(msg, sizeof msg, "%s: node %d is fixed (aprilsam_amd_node_set_fixed); this entry point does not take fixed nodes yet (DESIGN.md section 20)", who, i);
    set_last_error(ERR_UNSUPPORTED, msg);
    fprintf(stderr, "aprilsam_amd: ERROR %d: %s\n", (int)ERR_UNSUPPORTED, msg); fflush(stderr);
    return ERR_UNSUPPORTED;
}
// The entry points that do not take dense Gaussian factors: 0, or -12 with a message that names the first one.
// Nothing was read or written before; the param keeps its plan and factor.  A process that never made such a factor does not walk
static int refuse_gaussian(const char *who, const april_graph_t *g) {
    if (!g || !gaussian_ever() || g_opt.gaussian_on_host) return 0;
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    for (int i = 0, Fg = zsize(g->factors); i < Fg; i++) {
        if (fs[i]->type != APRILSAM_AMD_FACTOR_GAUSSIAN_TYPE || !gaussian_of(fs[i], nullptr, nullptr, nullptr)) continue;
        char msg[320];
        snprintf(msg, sizeof msg, "%s: factor %d is a dense Gaussian factor (aprilsam_amd_factor_gaussian_create); this entry point does not take them (DESIGN.md section 24)", who, i);
        set_last_error(ERR_UNSUPPORTED, msg);
        fprintf(stderr, "aprilsam_amd: ERROR %d: %s\n", (int)ERR_UNSUPPORTED, msg); fflush(stderr);
        return ERR_UNSUPPORTED;
    }
    return 0;
}
// the content check of the nodes' flags, once per call that linearises: a node fixed or freed since the last call is seen here
static void sync_fixed(GraphPack &gp, const april_graph_t *g) {
    if (gp.fx_nodes.empty() && !fixed_ever()) return;
    std::vector<int> now;
    scan_fixed(g, now);
    if (now != gp.fx_nodes) { gp.fx_nodes.swap(now); gp.fx_gen++; gp.fx_dirty = true; }
}
// the table -> device, after pack_factors: the records are rebuilt when the set or the packed endpoints changed
static void upload_fixed(GraphPack &gp) {
    if (gp.fx_nodes.empty()) { gp.fx_rec.clear(); gp.fx_dirty = false; return; }
    if (!gp.fx_dirty && gp.fx_topo == gp.topo_version) return;
    if (gp.fx_nodes.back() >= gp.N) fail(ERR_INTERNAL, "fixed node %d of %d packed nodes", gp.fx_nodes.back(), gp.N);
    std::vector<char> fx((size_t)gp.N, 0);
    for (int i : gp.fx_nodes) fx[i] = 1;
    std::vector<int2> rec;
    for (int f = 0; f < gp.F; f++) {
        const int a = gp.h_fa.p[f], b = gp.h_fb.p[f];
        const int m = (fx[a] ? FX_AA | FX_AB | FX_GA : 0) | (b >= 0 && fx[b] ? FX_AB | FX_BB | FX_GB : 0);
        if (m) rec.push_back(int2{ f, b >= 0 ? m : m & (FX_AA | FX_GA) });
    }
    if (!gp.fx_dirty && rec.size() == gp.fx_rec.size() && (rec.empty() || memcmp(rec.data(), gp.fx_rec.data(), rec.size() * sizeof(int2)) == 0)) { gp.fx_topo = gp.topo_version; return; }
    if (!gp.fx_dirty) gp.fx_gen++;
    gp.fx_rec.swap(rec);
    HIPCHECK(hipStreamSynchronize(gp.stream));      // (no launch that reads the old table is in flight when it is overwritten)
    gp.d_fx_nodes.need(gp.fx_nodes.size()); gp.d_fx_rec.need(std::max<size_t>(1, gp.fx_rec.size()));
    HIPCHECK(hipMemcpyAsync(gp.d_fx_nodes.p, gp.fx_nodes.data(), gp.fx_nodes.size() * 4, hipMemcpyHostToDevice, gp.stream));
    if (!gp.fx_rec.empty()) HIPCHECK(hipMemcpyAsync(gp.d_fx_rec.p, gp.fx_rec.data(), gp.fx_rec.size() * sizeof(int2), hipMemcpyHostToDevice, gp.stream));
    HIPCHECK(hipStreamSynchronize(gp.stream));      // (the sources are pageable)
    gp.fx_dirty = false; gp.fx_topo = gp.topo_version;
}
// the families' tables -> device (SideTable::upload): rows appended or edited since the last call, for the kernels of the step that follows
static void upload_tables(GraphPack &gp) { gp.mx.upload(gp.stream); gp.rb.upload(gp.stream); gp.pl.upload(gp.stream); gp.gs.upload(gp.stream); }
static void upload_factors(GraphPack &gp) {
    const int F = gp.F;
    if (F > gp.F_cap) {           // reallocation loses the old content: re-upload everything
        gp.F_cap = std::max(F, gp.F_cap + gp.F_cap / 2 + 64);
        gp.d_fa.need(gp.F_cap); gp.d_fb.need(gp.F_cap); gp.d_z.need((size_t)3 * gp.F_cap); gp.d_W.need((size_t)9 * gp.F_cap);
        gp.d_chi2f.need((size_t)gp.F_cap + REDUCE_PARTS);       // per-factor terms + the partial sums of device_chi2
        gp.F_on_device = 0; gp.lin_ctx = nullptr;        // (the weighted and selected slots of the last linearisation are gone with it)
    }
    const int f0 = gp.F_on_device;
    if (F > f0) {
        size_t n = F - f0;
        HIPCHECK(hipMemcpyAsync(gp.d_fa.p + f0, gp.h_fa.p + f0, n * 4, hipMemcpyHostToDevice, gp.stream));
        HIPCHECK(hipMemcpyAsync(gp.d_fb.p + f0, gp.h_fb.p + f0, n * 4, hipMemcpyHostToDevice, gp.stream));
        HIPCHECK(hipMemcpyAsync(gp.d_z.p + (size_t)3 * f0, gp.h_z.p + (size_t)3 * f0, n * 24, hipMemcpyHostToDevice, gp.stream));
        HIPCHECK(hipMemcpyAsync(gp.d_W.p + (size_t)9 * f0, gp.h_W.p + (size_t)9 * f0, n * 72, hipMemcpyHostToDevice, gp.stream));
    }
    const int d0 = gp.dirty_lo, d1 = std::min(gp.dirty_hi, f0);      // z / W of packed factors edited in place by the caller
    if (d1 > d0) {
        HIPCHECK(hipMemcpyAsync(gp.d_z.p + (size_t)3 * d0, gp.h_z.p + (size_t)3 * d0, (size_t)(d1 - d0) * 24, hipMemcpyHostToDevice, gp.stream));
        HIPCHECK(hipMemcpyAsync(gp.d_W.p + (size_t)9 * d0, gp.h_W.p + (size_t)9 * d0, (size_t)(d1 - d0) * 72, hipMemcpyHostToDevice, gp.stream));
    }
    gp.dirty_lo = gp.dirty_hi = 0;
    gp.F_on_device = F;
    gp.d_scalar.need(8); gp.h_scalar.need(8);
    upload_tables(gp);
}
// evaluate the host factors [from, end) through their vtable (aprilsam.c:156 calls factor->eval the same way) and form
// (J_a^T W) J_a, (J_a^T W) J_b, (J_b^T W) J_b, (J^T W) r in the reference's association (aprilsam.c:162-187)
static double eval_host_factors(GraphPack &gp, april_graph_t *g, int from) {
    const int nh = (int)gp.host_idx.size();
    gp.h_hostH.need((size_t)33 * std::max(nh, 1), true);
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    double chi2 = 0;
    // (the pairs of a factor with more than two nodes share one evaluation; the guard destroys the live one on every exit, the fail() paths included)
    struct EvalGuard { april_graph_factor_eval_t *e = nullptr; ~EvalGuard() { if (e) april_graph_factor_eval_destroy(e); } } guard;
    april_graph_factor_eval_t *&e = guard.e; int e_of = -1;
    std::vector<double> JtW;
    for (int k = from; k < nh; k++) {
        const int hp = gp.host_idx[k], gi = gp.p2g[hp];
        april_graph_factor_t *f = fs[gi];
        const int x = (int)((gp.vslot[hp] >> 8) & 0xff), y = (int)(gp.vslot[hp] & 0xff), carry = (int)(gp.vslot[hp] >> 16);
        if (gi != e_of) {
            if (e) { april_graph_factor_eval_destroy(e); e = nullptr; }
            e = f->eval(f, g, nullptr); e_of = gi;
            if (!e || !e->jacobians || !e->jacobians[0] || !e->W || !e->r) fail(ERR_BAD_GRAPH, "factor->eval returned an incomplete evaluation (aprilsam.h:75-89)");
            chi2 += e->chi2;
        }
        const int L = e->length;
        double *H = gp.h_hostH.p + (size_t)33 * k;
        memset(H, 0, 33 * 8);
        JtW.resize((size_t)3 * L);
        const int zs[2] = { x, y == 0xff ? -1 : y };
        for (int s0 = 0; s0 < 2; s0++) {
            const int z0 = zs[s0];
            if (z0 < 0) continue;
            const matd_t *J0 = e->jacobians[z0];
            if (!J0) fail(ERR_BAD_GRAPH, "factor->eval: fewer jacobians than nodes");
            if ((int)J0->nrows != L || J0->ncols != 3 || (int)e->W->nrows != L || (int)e->W->ncols != L)
                fail(ERR_UNSUPPORTED, "factor->eval: jacobians must be length x 3 and W length x length (3-DoF xyt nodes only, aprilsam.c:617)");
            for (int i = 0; i < 3; i++)
                for (int l = 0; l < L; l++) { double acc = 0; for (int m = 0; m < L; m++) acc += J0->data[m * 3 + i] * e->W->data[m * L + l]; JtW[(size_t)i * L + l] = acc; }
            for (int s1 = s0; s1 < 2; s1++) {
                const int z1 = zs[s1];
                if (z1 < 0) continue;
                if (s1 == s0 && !((carry >> s0) & 1)) continue;      // this node's diagonal block rides on another pair of the factor
                const matd_t *J1 = e->jacobians[z1];
                if (!J1) fail(ERR_BAD_GRAPH, "factor->eval: fewer jacobians than nodes");
                double *B = H + (s0 == 0 ? (s1 == 0 ? 0 : 9) : 18);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) { double acc = 0; for (int l = 0; l < L; l++) acc += JtW[(size_t)i * L + l] * J1->data[l * 3 + j]; B[i * 3 + j] = acc; }
            }
            if ((carry >> s0) & 1) {
                double *gv = H + 27 + 3 * s0;
                for (int i = 0; i < 3; i++) { double acc = 0; for (int l = 0; l < L; l++) acc += JtW[(size_t)i * L + l] * e->r[l]; gv[i] = acc; }
            }
        }
    }
    gp.host_evaluated = nh;
    return chi2;
}
static void upload_host_index(GraphPack &gp) {
    const int nh = (int)gp.host_idx.size();
    if (!nh) return;
    gp.d_host_idx.need(nh); gp.d_hostH.need((size_t)33 * nh);
    HIPCHECK(hipMemcpyAsync(gp.d_host_idx.p, gp.host_idx.data(), (size_t)4 * nh, hipMemcpyHostToDevice, gp.stream));
}

// states (and l_points) of all nodes -> pinned host -> device
static void pack_states(GraphPack &gp, const april_graph_t *g, bool with_lp, bool upload = true) {
    const int N = zsize(g->nodes);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    if ((size_t)3 * N > gp.h_state.cap || (size_t)3 * N > gp.h_lp.cap || (size_t)3 * N > gp.d_state.cap || (size_t)3 * N > gp.d_lp.cap) gp.mirror_sync = false;   // (a buffer is about to move)
    gp.h_state.need((size_t)3 * N); gp.h_lp.need((size_t)3 * N); gp.h_dx.need((size_t)3 * N);
    for (int i = 0; i < N; i++) {
        if (i + 8 < N) __builtin_prefetch(ns[i + 8]->state);
        const april_graph_node_t *n = ns[i];
        if (n->type != APRIL_GRAPH_NODE_XYT_TYPE || n->length != 3) fail(ERR_UNSUPPORTED, "node %d: only xyt nodes (type 100, 3 DoF) are supported (aprilsam.h:94)", i);
        memcpy(gp.h_state.p + (size_t)3 * i, n->state, 24);
        if (with_lp) memcpy(gp.h_lp.p + (size_t)3 * i, n->l_point, 24);
    }
    gp.N = N;
    gp.pending.clear();           // (every state goes to the device below, or through k_load_states: nothing is left behind the mirrors)
    gp.d_state.need((size_t)3 * N); gp.d_lp.need((size_t)3 * N); gp.d_dx.need((size_t)3 * N);
    if (!upload) return;          // (the batch step reads the pinned mirror from its first kernel, k_load_states)
    HIPCHECK(hipMemcpyAsync(gp.d_state.p, gp.h_state.p, (size_t)24 * N, hipMemcpyHostToDevice, gp.stream));
    if (with_lp) HIPCHECK(hipMemcpyAsync(gp.d_lp.p, gp.h_lp.p, (size_t)24 * N, hipMemcpyHostToDevice, gp.stream));
}

// Incremental steps: compare every node's state / l_point with the pinned mirrors, copy what differs and list those poses
// (gp.changed) -- typically the new pose, the poses the previous step updated, whatever the caller moved.  Returns true when
// patching the listed poses brings the device arrays up to date; false when a full load is needed (mirrors and device not
// known to agree, a buffer had to grow, or too many poses changed for patches to pay).
static long long g_full_reason[4] = { 0 };      // APRILSAM_AMD_INC_PROFILE: why a step loaded every state (mirrors not in step / own updates / caller's changes), steps
static bool pack_states_diff(GraphPack &gp, const april_graph_t *g) {
    const int N = zsize(g->nodes);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    bool full = !gp.mirror_sync || (size_t)3 * N > gp.d_state.cap || (size_t)3 * N > gp.d_lp.cap || (size_t)3 * N > gp.d_dx.cap;
    gp.h_state.need((size_t)3 * N, true); gp.h_lp.need((size_t)3 * N, true); gp.h_dx.need((size_t)3 * N); gp.h_out.need((size_t)3 * N);
    gp.d_state.need((size_t)3 * N); gp.d_lp.need((size_t)3 * N); gp.d_dx.need((size_t)3 * N);
    gp.changed.clear();
    const int Nold = full ? 0 : gp.N;
    for (int i = 0; i < N; i++) {
        if (i + 8 < N) __builtin_prefetch(ns[i + 8]->state);
        const april_graph_node_t *n = ns[i];
        if (n->type != APRIL_GRAPH_NODE_XYT_TYPE || n->length != 3) fail(ERR_UNSUPPORTED, "node %d: only xyt nodes (type 100, 3 DoF) are supported (aprilsam.h:94)", i);
        double *ms = gp.h_state.p + (size_t)3 * i, *ml = gp.h_lp.p + (size_t)3 * i;
        if (i >= Nold || memcmp(ms, n->state, 24) != 0 || memcmp(ml, n->l_point, 24) != 0) {
            memcpy(ms, n->state, 24); memcpy(ml, n->l_point, 24);
            gp.changed.push_back(i);
        }
    }
    gp.N = N;
    // poses the previous step updated itself (apply_visits brought their mirrors up to date: the walk above found them equal):
    // the device copy of their state is what is stale
    g_full_reason[3]++;
    if (full) g_full_reason[0]++;
    if (!full) {
        if (gp.pending.size() > 48) { full = true; g_full_reason[1]++; }
        else for (int i : gp.pending) if (i < N && std::find(gp.changed.begin(), gp.changed.end(), i) == gp.changed.end()) gp.changed.push_back(i);
    }
    gp.pending.clear();
    if (!full && gp.changed.size() > 48) { full = true; g_full_reason[2]++; }
    return !full;
}

// The same for a step whose walk visits only a few poses (aprilsam.c:755-771, naffected <= 5): what the step READS are the
// l_points / states of the poses of its new factors and of the poses it visits, plus the new poses -- only those are compared
// with the mirrors and patched.  The cost of a step then no longer grows with the size of the graph (the full walk is 1 ns per
// pose per step: 3.5 us on M3500, 100 us on a 100 k-pose graph).  Invariant kept: device arrays == mirrors for EVERY pose;
// mirror == host object only for the poses some call has looked at since -- every consumer that needs all of them (batch
// steps, chi^2, full walks, re-plans) walks all node objects itself.
static bool pack_states_some(GraphPack &gp, const april_graph_t *g, const std::vector<int> &involved) {
    const int N = zsize(g->nodes);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    if (!gp.mirror_sync || (size_t)3 * N > gp.d_state.cap || (size_t)3 * N > gp.d_lp.cap || (size_t)3 * N > gp.d_dx.cap || (size_t)3 * N > gp.h_state.cap ||
        (size_t)3 * N > gp.h_lp.cap || (size_t)3 * N > gp.h_dx.cap || (size_t)3 * N > gp.h_out.cap || N < gp.N) return pack_states_diff(gp, g);
    gp.changed.clear();
    auto look = [&](int i, bool is_new) {
        const april_graph_node_t *n = ns[i];
        if (n->type != APRIL_GRAPH_NODE_XYT_TYPE || n->length != 3) fail(ERR_UNSUPPORTED, "node %d: only xyt nodes (type 100, 3 DoF) are supported (aprilsam.h:94)", i);
        double *ms = gp.h_state.p + (size_t)3 * i, *ml = gp.h_lp.p + (size_t)3 * i;
        if (is_new || memcmp(ms, n->state, 24) != 0 || memcmp(ml, n->l_point, 24) != 0) {
            memcpy(ms, n->state, 24); memcpy(ml, n->l_point, 24);
            if (std::find(gp.changed.begin(), gp.changed.end(), i) == gp.changed.end()) gp.changed.push_back(i);
        }
    };
    for (int i = gp.N; i < N; i++) look(i, true);
    const int Nold = gp.N;
    for (int i : involved) if (i >= 0 && i < Nold) look(i, false);
    gp.N = N;
    g_full_reason[3]++;
    bool full = false;
    if (gp.pending.size() > 48) { full = true; g_full_reason[1]++; }
    else for (int i : gp.pending) if (i < N && std::find(gp.changed.begin(), gp.changed.end(), i) == gp.changed.end()) gp.changed.push_back(i);
    gp.pending.clear();
    if (!full && gp.changed.size() > 48) { full = true; g_full_reason[2]++; }
    return !full;
}

// evaluation points of the unary factors [from, to): the node's state as packed by this call (april_graph_xytpos.c:83-85
// reads node->state when the factor is evaluated, and the reference evaluates a factor exactly once between batch steps)
static void record_unary_points(GraphPack &gp, int from, int to, const double *states) {
    gp.h_upt.resize((size_t)3 * gp.F, 0.0);
    for (int f = from; f < to; f++) if (gp.h_fb.p[f] < 0) memcpy(&gp.h_upt[(size_t)3 * f], states + (size_t)3 * gp.h_fa.p[f], 24);
}

