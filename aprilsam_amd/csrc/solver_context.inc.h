// solver_context.inc.h -- part of solver.hip.cpp (ONE translation unit: the kernels of kernels.hip.h are compiled once); included from there,
// inside namespace asam.  Contents: the solver context of a param (plan, device tables, fronts, captured graphs), the failure path, plan upload with its launch tables, the step counter, plan reuse and the orientation of asymmetric factors (the launches themselves: solver_launch.inc.h).
// ------------------------------------------------------------------------------------------------------
// solver context — one per april_graph_cholesky_param_t pointer
// ------------------------------------------------------------------------------------------------------
enum { K_LINEARIZE = 0, K_FRONT_SMALL, K_ASSEMBLE_BIG, K_PANEL_BIG, K_SYRK_BIG, K_BACKSOLVE, K_UPDATE, NKERN };      // K_PANEL_BIG = k_block_chain + k_block_solve, K_SYRK_BIG = k_syrk_big + k_syrk_big32, K_BACKSOLVE = every back-substitution kernel
static const char *const KNAMES[NKERN] = { "k_linearize", "k_front_small", "k_assemble_big", "k_panel_big", "k_syrk_big", "k_backsolve", "k_update_states" };
struct Launch { int list_off, pre_off, n, grid; bool single = false; int tile = TILE; };   // single: every front has exactly one work item     // offsets into the int launch-table buffer

struct LevelPlan {
    int small_off = 0, n_small = 0; size_t small_lds = 0;      // fronts handled by k_front_small
    long long full_limit = 0;                                  // ... fully in LDS when their array fits this many bytes, else panel mode
    int small_nt = 512;                                        // ... with this many threads per workgroup
    int n_big = 0; size_t asm_lds = 0;
    Launch asm_big{};                                          // k_assemble_big (chunks of block columns)
    std::vector<Launch> syrka, syrk1;                          // paired outer blocks (option syrk_pair_tiles; empty: every block closes with syrkw): after the FIRST block of a pair the "ahead" update of the fronts that have a second one, and the single-block wide update of the fronts that end here; syrkw then holds the K = 256 update after the second block
    bool paired = false;
    std::vector<Launch> bchain, btile, syrkw;                  // per 128-column outer block: diagonal-block workgroups, row tiles (Launch::tile = rows per wave / 16), the wide update that closes it (Launch::tile = output tile)
    int all_off = 0, n_all = 0; size_t solve_lds = 0;          // every front (k_backsolve)
    size_t solve_w_lds = 0; int maxns = 0;                     // ... in the column-per-lane form (k_backsolve_w: L panel in LDS), widest own part
    Launch bs_gemv{};                                          // fronts whose update-row product is spread over workgroups first (k_backsolve_gemv)
    Launch bs_blk{}; size_t bs_blk_lds = 0;                    // wide fronts back-substituted by a chain + helper workgroups (k_backsolve_blk); grid 0: none
    int rest_off = 0, n_rest = 0; size_t rest_lds = 0;         // ... and the level's other fronts (k_backsolve_t)
};

// state of the incremental fast path (inc_fast.*): the plan of the last batch step stays frozen, poses added since
// form one growing TAIL front at the root, and only fronts on the root paths of changed leaves are regenerated
struct IncState {
    bool ready = false;                     // helper tables below are built for the current base plan
    bool pristine = false;                  // ... and no incremental / extended-plan step has touched them since (inc_prepare need not run again for the same plan)
    int Nb = 0, Fb = 0, nF0 = 0, nLev0 = 0;
    int cap_nodes = 0, cap_fact = 0;         // slack reserved at plan upload (0 until the param has seen an incremental call)
    long long i32_used = 0, dest_used = 0, child_used = 0, tab_used = 0, pool_used = 0, pool_cap = 0, o_rows = 0, o_rel = 0;
    int slots_used = 0;
    std::vector<FrontDesc> fd;              // host mirror of the device descriptors (base fronts, then TAIL)
    std::vector<int> pos_front;             // base position -> base front
    std::vector<int> parent;                // current assembly parent (base roots get TAIL once they see tail rows)
    std::vector<std::vector<int>> E;        // per base front: tail nodes in its extended struct (sorted)
    std::vector<std::vector<int>> xfac;     // per front (TAIL = index nF0): factors added since the batch
    std::vector<int> bf_ptr, bf_idx;        // base factors owned by each base front (CSR)
    std::vector<int> rel_begin;             // per front: absolute offset of its current child->parent block map
    std::vector<int> cur_nub;               // per front: current update blocks
    std::vector<long long> cur_cap;         // per front: doubles allocated at fd.off
    std::vector<char> dirty;
    std::vector<int> f_level;               // base levels, tail front i = nLev0 + i
    int zpos = 0;                           // a position whose x entries stay zero: what the phantom rows of the last tail front point at
    int tail_ok = -1;                       // tail front whose factor on the device is complete in the padded layout (candidate for tail_refactor), or -1
    int recs_stale = -1;                    // tail front whose destination records on the device lack the factors tail_refactor took in directly, or -1
    std::vector<int> t_first, t_cnt;        // tail fronts: first pose id, own poses
    std::vector<int> tf_of;                 // tail pose (id - Nb) -> its tail front
    std::vector<std::vector<int>> kids;     // per front: children that are NOT in the base plan's child lists (children of tail fronts)
    std::vector<LevelPlan> base_levels;     // launch tables of all fronts per level for the back substitution
    // staging for the per-step uploads (members: the async copies read them until the step's final sync)
    std::vector<int> st_i32, st_tab, st_sb, st_sr, st_ids; std::vector<DestRec> st_dest; std::vector<ChildRec> st_child;
    std::vector<unsigned char> st_sw; std::vector<double> st_zeros; std::vector<char> need;
    // low-rank updates of the fronts on a loop closure's root path (front_update_body, option inc_update)
    std::vector<char> stale;                // per front: its destination / child records on the device lack what update steps folded in directly
    bool upd_ok = true;                     // false after a step that failed half-way, until the next full plan
    bool base_has_big = false;              // the base plan has fronts on the multi-workgroup path
    std::vector<char> st_mid, st_mode; std::vector<int> st_owner, st_mask, st_wout, st_slot; std::vector<UpdRec> st_upd, st_rec;
    // what the last april_graph_cholesky_inc did, as aprilsam_amd_debug_inc_forms hands it out (IF_HEAD ints, then IF_ROW per dirty front); empty: none yet
    std::vector<int> forms;
};
// aprilsam_amd_debug_inc_forms: header and row widths, the path codes of header [3]
constexpr int IF_HEAD = 14, IF_ROW = 10 + UPD_MAXC;
enum { IF_REPLAN = 0, IF_TAIL_SOLVE = 1, IF_TAIL_LIST = 2, IF_TAIL_GENERAL = 3, IF_ONE = 4, IF_MULTI = 5, IF_LEVELS = 6 };
static void inc_forms_head(IncState &I, int path, int fail, int n_fac, const TailStep &ts, int n_old, int threads, int one, int up_multi, int dn_multi) {
    int h[IF_HEAD] = { 0, IF_HEAD, IF_ROW, path, fail, n_fac, ts.t >= 0 ? ts.a_idx : -1, ts.t >= 0 ? n_old : -1, ts.t >= 0 ? ts.nsb : -1, ts.t >= 0 && ts.solve ? ts.s_idx : -1,
                       threads, one, up_multi, dn_multi };
    I.forms.assign(h, h + IF_HEAD);
}
static void inc_forms_row(IncState &I, int t, int mode, int nsb, int nub, int old_nub, int inplace, int mid, const UpdRec *u) {
    int r[IF_ROW] = { t, mode, nsb, nub, old_nub, u ? u->mask : 0, u ? u->n_own : 0, u ? u->n_ch : 0, inplace, mid };
    for (int k = 0; k < UPD_MAXC; k++) r[10 + k] = u && k < u->n_ch ? u->ch_cnu[k] : -1;
    I.forms.insert(I.forms.end(), r, r + IF_ROW);
    I.forms[0]++;
}

// The work-entry tables of the retained-factor consumers: one vector of entries per table, and per level and kernel the run of entries
// its launch takes.  span_of(ent, fill): the run that fill() appends to ent.
struct Span { int off = 0, n = 0; };
template <class E, class Fill> static Span span_of(std::vector<E> &ent, Fill fill) {
    Span sp{ (int)ent.size(), 0 };
    fill();
    sp.n = (int)ent.size() - sp.off;
    return sp;
}

// marginal covariances (solver_marginals.inc.h): per level, the runs of its work entries in the selected inversion's table
struct SelLevel { Span gat, diag, tri, x, sus, sss; };

// The structure the retained factor lives in, derived once for all its readers (factor_view, solver_query.inc.h: builder and validity rule):
// the fronts (scr: written by the selected inversion's table builder, read by its kernels alone), their depth below the root, the fronts of
// every depth (root first), i32 = pos | pos_front (node -> elimination position, position -> owning front) of the N nodes with its one
// device copy, the end of the pool the fronts occupy and the estimated flops of the selected inversion
struct FactorView {
    long long gen = 0;                     // grows with every rebuild: what the readers' own tables are kept against
    int kind = 0; long long serial = -1;   // FACT_* and fact_serial it was built for (kind 0: none)
    int N = 0; long long pool_end = 1; double flops = 0;
    std::vector<SelFront> fr; std::vector<int> depth, i32; std::vector<std::vector<int>> lev;
    DBuf<int> d_i32; bool on_device = false;
    void release() { d_i32.release(); fr.clear(); depth.clear(); i32.clear(); lev.clear(); kind = 0; serial = -1; on_device = false; }
};

// A front of the view as the solve kernels take it (pathsolve.hip.h, treesolve.hip.h): its local vectors at buf, ncol columns wide, under
// the record `parent`, its columns mapped to the parent's through the column map at cmap
static PsFront ps_front(const SelFront &F, long long buf, int ncol, int parent, int cmap) {
    return PsFront{ F.off, buf, F.s, F.u, F.R, ncol, parent, F.rel_begin, cmap, F.first };
}

// joint covariances of any pair and gating (solver_gating.inc.h): the scratch maps of one call, and the device buffers of the path solves
struct PathState {
    long long gen = -1;                    // FactorView::gen the scratch maps are sized for
    std::vector<int> rec, node_j;          // rec: front -> record, node_j: node -> column group (both -1 between calls)
    DBuf<PsFront> d_fr; DBuf<int4> d_ent; DBuf<int> d_cmap; DBuf<long long> d_at; DBuf<PsPath> d_path; DBuf<PsPair> d_pair;
    DBuf<double> d_buf, d_cov, d_in; HBuf<double> h_out;
    DBuf<int> d_pidx;                      // k_gate_polar: candidate -> its pair's block in d_cov
    DBuf<int> d_jtab; DBuf<long long> d_joff;      // k_block_chol: hyp_ptr | tab_ptr | the index table; the matrices' offsets
    DBuf<LdEnt> d_ldent; DBuf<double> d_ldpart; DBuf<int> d_ldbad; HBuf<double> h_ld;      // k_logdet_partial / k_logdet_sum: the entries, the partials, the counts; the result
    long long ld_gen = -1; int ld_n = 0;   // FactorView::gen d_ldent describes, and its entries
    long long peak_doubles = 0;            // the largest work buffer a chunk has used
    void release() {
        d_fr.release(); d_ent.release(); d_cmap.release(); d_at.release(); d_path.release(); d_pair.release(); d_buf.release(); d_cov.release(); d_in.release(); h_out.release(); d_pidx.release(); d_jtab.release(); d_joff.release();
        d_ldent.release(); d_ldpart.release(); d_ldbad.release(); h_ld.release(); ld_gen = -1; ld_n = 0;
        rec.clear(); node_j.clear(); gen = -1;
    }
};

// solves with the retained factor (solver_treesolve.inc.h): the tables of the whole-tree passes, kept against the view's generation,
// and the device / pinned buffers of one call
struct TsLevel { Span assemble, trsm, gemm, gather, gemmt; };
struct TreeState {
    long long gen = -1;                    // FactorView::gen the tables describe
    long long rows = 0;                    // sum over the fronts of s + u: the work buffer takes this many doubles per column
    std::vector<int> wrow; std::vector<TsLevel> lev;      // a front's first row in the work buffer; the levels, root first
    DBuf<PsFront> d_fr; DBuf<int2> d_ent; DBuf<int> d_cptr, d_npos, d_nodes; DBuf<TsKid> d_cent;
    DBuf<double> d_buf, d_B, d_st; HBuf<double> h_B, h_X;
    long long peak_bytes = 0;              // the largest work buffer a call has used
    void release() {
        d_fr.release(); d_ent.release(); d_cptr.release(); d_npos.release(); d_nodes.release(); d_cent.release();
        d_buf.release(); d_B.release(); d_st.release(); h_B.release(); h_X.release();
        wrow.clear(); lev.clear(); gen = -1;
    }
};

struct Context {
    Plan plan;
    bool have_plan = false;
    std::vector<int> pat;                 // factor node ids the plan was built for (2 per factor)
    int patN = 0;
    // device copies of the plan
    DBuf<int> d_i32; DBuf<FrontDesc> d_fd; DBuf<DestRec> d_dest; DBuf<ChildRec> d_child; DBuf<double> d_lambda;
    DevPlan dp{};
    DBuf<int> d_tab;                      // launch tables
    std::vector<LevelPlan> levels;
    DBuf<unsigned char> d_swap;
    DBuf<int> d_pos;
    DBuf<long long> d_prof;
    // numeric state
    DBuf<double> d_pool, d_H, d_x, d_diag;   // d_diag: factored diagonal blocks of the current panel step, one per active big front
    DBuf<int> d_bad;
    HBuf<int> h_bad;
    IncPrologue pro{}; InlinePatches inl{};       // arguments of the incremental step's first kernel
    bool no_speculation = false;          // batch_impl: the next call reads the factor objects before it launches (set when a speculative run was voided)
    HBuf<long long> h_kstamp; HBuf<int> h_done; int done_seq = 0, one_wait = 0;      // k_inc_one: phase stamps (profile), completion word the host spins on
    std::vector<double> h_lambda;
    aprilsam_amd_stats_t st{};
    hipEvent_t ev[8] = {};
    bool have_events = false;
    // per-kernel HIP-event timing (instrumented passes only)
    double k_ms[NKERN] = {}; long long k_calls[NKERN] = {};
    std::vector<hipEvent_t> k_ev; std::vector<int> k_ids, k_lev;
    std::vector<double> lev_up_ms, lev_dn_ms;       // ... the same event pairs summed per level of the assembly tree (factorisation / back substitution)
    // incremental bookkeeping (aprilsam.c:741-751, 566-575)
    bool have_fact = false;               // a batch factorisation exists (reference: param->chol != NULL)
    int plan_pin = 0;                     // pin_last the plan was built with
    long long plan_persist = 0;           // launch_table_key() the launch tables were built with
    int same_topo_batches = 0;            // batch calls on an extended (base + tail fronts) plan whose topology did not change since the previous call
    bool used_inc = false;                // april_graph_cholesky_inc has been called on this param
    bool want_inc = false;                // the param has been used incrementally: plan uploads reserve the append slack
    int batch_nodes = 0;                  // #nodes at the last batch step (those carry the Tikhonov term)
    IncState inc;
    int inc_F = 0, inc_N = 0;                      // factors / nodes folded into the factorisation so far
    std::vector<RefModel::Visit> visits; std::vector<int> involved;
    std::vector<int> base_tab;                     // host copy of the launch tables of the base plan
    std::vector<int> inc_slot_blk, inc_slot_rhs;   // slots of the factors added since the base plan (3 / 2 per factor)
    long long pat_serial = -1, pat_topo = -1;      // the pack (serial) and its topo_version at which `pat` last equalled the packed endpoints (prepare_plan)
    RefModel model;                       // the reference's tree / counters (refmodel.cpp), rebuilt lazily after a batch
    PatchList patches;                    // per-step table updates of the incremental fast path
    int batch_factors = 0;                // #factors at the last batch step
    // Factors with an information matrix that is not symmetric as given (GraphPack::asym): wt[f] = 1 when the reference eliminates endpoint b
    // before endpoint a, i.e. when the block it accumulates is J_b^T W J_a (aprilsam.c:171,520: upper triangle of ITS order only) and not
    // J_a^T W J_b -- the two are transposes of each other only for a symmetric W.  Fixed when the factor enters the system: at a batch call
    // for every factor (the reference re-orders everything), at an incremental call for the new ones (old poses keep their positions, new
    // ones are appended, aprilsam.c:393-396).  Travels to the device as bit 1 of the per-factor swap byte (k_linearize).
    std::vector<unsigned char> wt; bool wt_any = false, wt_dirty = false;
    long long wt_serial = -1, wt_topo = -1, wt_content = -1;
    DBuf<long long> d_guard; DBuf<int> d_guard_cnt; int n_guard = 0, guard_len = 0;      // option pool_guard: offsets of the guard bands in d_pool
    std::vector<unsigned char> swap_host;          // host copy of d_swap's base-plan part (the source of an asynchronous copy: must outlive it)
    // captured numeric phase
    // multi-level ("persistent") launches of the batch path: the top levels of the tree, where a level holds only a handful
    // of fronts, run as ONE launch for the factorisation and ONE for the back substitution, fronts waiting on per-front
    // dependency flags instead of on kernel boundaries (kernels.hip.h: wait_flag / publish_flag)
    int persist_l0 = -1;                  // first level of the multi-level launch, -1: none
    int persist_dn_l0 = -1;               // ... of the back substitution's: persist_l0, or 0 where level 0 joins that launch alone (option persist_leaves; upload_plan)
    int p_up_off = 0, p_up_n = 0, p_dn_off = 0, p_dn_n = 0, p_nt = 1024; size_t p_up_lds = 0, p_dn_lds = 0; long long p_up_full = 0; int p_dn_maxns = 0, p_dn_maxnu = 0;      // (p_dn_maxnu: tallest update block, rows, of the back substitution's list)
    int x_up_off = 0, x_up_n = 0, x_dn_off = 0, x_dn_n = 0;      // the same two lists in XCD-placed order (option xcd_place; x_up_n = 0: not placed)
    int x_leaf_off = 0, x_leaf_n = 0;                           // ... and level 0's fronts for its two launches (x_leaf_n = 0: level 0 keeps its own list)
    int persist_up_l0 = -1;               // first level of the factorisation's multi-level launch: persist_l0, or 0 where level 0 joins that launch too (option persist_up; upload_plan)
    int u_off = 0, u_n = 0, u_fronts = 0; // ... and the list it runs (empty slots included), in the order option persist_up asks for; u_fronts: its fronts
    DBuf<int> d_flags, d_flevel, d_perm, d_epoch, d_marks;   // d_epoch: the step counter every dependency flag carries (kernels.hip.h wait_flag); d_marks: fronts regenerated by an incremental step
    DBuf<uint4> d_xg;                     // x as epoch-tagged granules, one per entry of d_x: the hand-over inside the multi-level back substitutions (kernels.hip.h: gather_x; option tagged_x)
    int flag_stride = 0;                  // d_flags = three arrays of this many words: "factor done", "x done", "vectors ready" per front
    long long epoch_steps = 0;            // numeric phases enqueued since the counter was (re)started (rewind_epoch)
    DBuf<double> d_dinv, d_bsb_far; DBuf<int> d_bsb_flags;   // inverse diagonal blocks of the big fronts; scratch of k_backsolve_blk
    DBuf<int> d_solve_tab; std::vector<int> solve_tab;      // april_graph_cholesky_inc_solver: front lists of its back substitution
    DBuf<UpdRec> d_upd; DBuf<double> d_wbuf;               // incremental steps: update records per launch-list entry, the step's travelling vectors
    DBuf<double> d_lm_trial, d_lm_hacc, d_lm_terms, d_lm_trace; DBuf<LmScalars> d_lm; HBuf<LmScalars> h_lm;
    // chordal initialisation (solver_chordal.inc.h): [scratch of the state update 3N][theta N][4 scalars]; the components chosen for the max factors
    DBuf<double> d_ch; HBuf<double> h_ch; DBuf<int> d_ch_sel;
    long long n_captures = 0;                      // hipGraphs captured and instantiated for this context so far (aprilsam_amd_debug_graph_captures)
    // captured graphs that are no longer current: hipGraphExecDestroy takes 0.24 ms on this stack, so they are destroyed while the
    // GPU works on a step (reap_retired), not on the way to the next plan
    // A retired graph may still have launches in flight (resident / sharded loops enqueue steps without a sync in between): it carries an
    // event recorded on the stream it was last launched on and is destroyed only once that event has completed.
    struct Retired { hipGraphExec_t g; hipEvent_t done; };
    std::vector<Retired> retired;
    hipStream_t graph_stream = nullptr;            // the stream a captured graph was last launched on (replay_captured)
    void reap_retired(bool wait = false) {
        size_t keep = 0;
        for (Retired &r : retired) {
            if (r.done) {
                if (wait) (void)hipEventSynchronize(r.done);
                else if (hipEventQuery(r.done) != hipSuccess) { retired[keep++] = r; continue; }
                (void)hipEventDestroy(r.done);
            }
            (void)hipGraphExecDestroy(r.g);
        }
        retired.resize(keep);
    }
    void retire(hipGraphExec_t &g) {
        if (!g) return;
        if (retired.size() >= 8) reap_retired();                   // (bounded: call sequences that never reach a reaping point)
        if (retired.size() >= 32) reap_retired(true);              // (... and whose launches never finish in between)
        Retired r{ g, nullptr };
        if (graph_stream && hipEventCreateWithFlags(&r.done, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(r.done, graph_stream) != hipSuccess) { (void)hipEventDestroy(r.done); r.done = nullptr; }
        } else r.done = nullptr;
        retired.push_back(r); g = nullptr;
    }
    // One captured hipGraph: the exec handle, the key it was captured with (GraphPack::capture_key plus this graph's extras) and how many
    // runs that key has seen.  fit() is the whole staleness rule: another key retires the graph; it returns whether this run replays
    // (or captures) one.  skip_first: a graph is worth its capture, instantiation and destruction (0.3 ms together) only if the
    // configuration comes back, so the first run with a new key enqueues its kernels directly
    struct Captured {
        const bool skip_first; hipGraphExec_t exec = nullptr; CaptureKey key; long long runs = 0;
        Captured(bool skip_first = false) : skip_first(skip_first) {}
        bool fit(Context &c, const CaptureKey &k) {
            if (!(k == key)) { c.retire(exec); key = k; runs = 0; }
            return runs++ > 0 || !skip_first;
        }
    };
    // The numeric phase of a resident step.  Extras: none.  N is not in the key: this graph runs only behind resident_begin_impl, whose
    // prepare_plan makes a new plan when N differs from the pattern's (upload_plan retires every capture); the re-planned incremental
    // step (unary_at_lp) is never captured.  gc_gen is not in it: gc_n > 0 only inside aprilsam_amd_optimize_gnc, which enqueues LM
    // iterations (cap_lm) and never this phase
    Captured cap_step;
    // The same phase as the API call runs it: first kernel reads the caller's states from the pinned mirror, last kernel writes new
    // states / dx / pivot flag back to pinned mirrors -- one graph launch + one stream sync per call.  Extras: those four mirrors
    // (h_state, h_lp, h_dx, h_bad) and N, the length k_load_states copies.  No gc_gen, as above
    Captured cap_api{ true };
    // Levenberg-Marquardt (solver_lm.inc.h): one iteration.  Extras: the four LM buffers it reads, N (the lengths of k_lm_commit and
    // k_lm_norms) and gc_gen -- a GNC run's candidates table serves that run alone
    Captured cap_lm;
    void retire_captures() { for (Captured *g : { &cap_step, &cap_api, &cap_lm }) { retire(g->exec); g->runs = 0; } }
    double lambda_val = -1; int lambda_N = -1;     // what d_lambda currently holds (uniform batch value), -1: unknown
    long long lambda_fx_gen = 0, lambda_fx_serial = 0;      // ... apart from the 1.0 of the fixed nodes of this pack at this fx_gen (k_fix_mask; set_lambda)
    DBuf<int> d_fx_mask;                           // ... and which nodes of a covariance query are among them (k_fix_cov)
    std::vector<int> fact_fixed;                   // the fixed nodes the retained factor was made with (record_factor)
    // marginal covariances (solver_marginals.inc.h): what the last successful solver call left in d_pool (FACT_*), at which value of
    // epoch_steps; the Sigma pool (front pool layout) and the step it was computed for; launch tables kept against the view's generation
    int fact_kind = 0; long long fact_epoch = -1; bool fact_asym = false;
    long long fact_pack = -1; bool fact_upt = false;      // the pack (GraphPack::serial) the factorised system was linearised from; its priors were linearised at d_upt (factor audit)
    bool resident_stepped = false;                 // the current resident loop has enqueued a step (its failure record means something)
    bool resident_failed = false;                  // a step of the current resident loop met a non-positive pivot (resident_sync saw it): resident_end writes nothing
    bool resident_open = false;                    // between aprilsam_amd_resident_begin and _end: the consumers of the retained factor answer -1 (no_retained_factor)
    DBuf<double> d_sigma, d_sel_scr; DBuf<SelFront> d_sel_fd; DBuf<int> d_sel_q; DBuf<int4> d_sel_ent; HBuf<double> h_cov;
    long long fact_serial = 0;                     // factorisations recorded so far (only grows)
    std::vector<SelLevel> sel_levels;
    long long sel_serial = -1, sel_tab_gen = -1, sel_runs = 0;      // sel_serial: the factorisation Sigma was computed for; sel_tab_gen: FactorView::gen of the tables
    FactorView view;
    PathState ps;
    TreeState ts;
    void release_sel() {
        d_sigma.release(); d_sel_scr.release(); d_sel_fd.release(); d_sel_q.release(); d_sel_ent.release(); h_cov.release();
        sel_levels.clear(); sel_serial = -1; sel_tab_gen = -1;
        view.release(); ps.release(); ts.release();
    }
    void release() {
        release_sel();
        d_i32.release(); d_fd.release(); d_dest.release(); d_child.release(); d_lambda.release(); d_fx_mask.release(); d_tab.release(); d_swap.release(); d_pos.release();
        d_pool.release(); d_H.release(); d_x.release(); d_diag.release(); d_bad.release(); h_bad.release(); patches.release();
        h_done.release(); h_kstamp.release(); d_prof.release(); d_upd.release(); d_wbuf.release(); d_flags.release(); d_flevel.release(); d_epoch.release(); d_marks.release(); d_perm.release(); d_solve_tab.release(); d_dinv.release(); d_bsb_far.release(); d_bsb_flags.release(); d_guard.release(); d_guard_cnt.release(); n_guard = 0;
        d_lm_trial.release(); d_lm_hacc.release(); d_lm_terms.release(); d_lm_trace.release(); d_lm.release(); h_lm.release();
        d_ch.release(); h_ch.release(); d_ch_sel.release();
        retire_captures(); reap_retired(true);
        if (have_events) for (auto &e : ev) (void)hipEventDestroy(e);
        have_events = false;
        for (auto &e : k_ev) (void)hipEventDestroy(e);
        k_ev.clear();
    }
};
static Registry<Context> g_ctx;

static void forget_stream(hipStream_t s) {
    g_ctx.for_each([&](Context &c) { if (c.graph_stream == s) c.graph_stream = nullptr; });
}

static Context &ctx_for(const april_graph_cholesky_param_t *p) {
    auto it = g_ctx.find(p);
    if (it == g_ctx.end()) it = g_ctx.emplace(p, std::make_unique<Context>()).first;
    return *it->second;
}
void drop_context(const april_graph_cholesky_param_t *p) {
    SlotLock lk(p, nullptr);
    auto it = g_ctx.find(p);
    if (it != g_ctx.end()) { it->second->release(); g_ctx.erase(it); }
}
// the debug counters and their like: one field of the param's context, or -1 for a param without one
template <class F> static long long context_field(const april_graph_cholesky_param_t *p, F f) {
    SlotLock lk(p, nullptr);
    auto it = g_ctx.find(p);
    return it == g_ctx.end() ? -1 : (long long)f(*it->second);
}
bool get_stats(const april_graph_cholesky_param_t *p, aprilsam_amd_stats_t *out) {
    SlotLock lk(p, nullptr);
    auto it = g_ctx.find(p);
    if (it == g_ctx.end()) return false;
    *out = it->second->st;
    return true;
}

// ------------------------------------------------------------------------------------------------------
// failure path (errors.h): every entry point below runs its body inside guarded().  A SolverError thrown anywhere under
// it unwinds to here (the body's lock_guard is released on the way): message on stderr, code kept for
// aprilsam_amd_last_error / stats.error_code, and the solver state that may be half-built -- the graph's pack, the param's
// plan, fronts, captured graphs, sharding state -- is dropped wholesale, exactly as param_destory / graph_destroy would.
// The caller's node objects are only ever written after a call's final stream sync succeeded, so they are untouched.
// ------------------------------------------------------------------------------------------------------
struct ShardState;
static void drop_shard_state(const void *param);
static void on_failure(const april_graph_cholesky_param_t *param, const april_graph_t *g, int code, const std::string &msg) {
    set_last_error(code, msg);
    fprintf(stderr, "aprilsam_amd: ERROR %d: %s -- node states left untouched\n", code, msg.c_str());
    fflush(stderr);
    SlotLock lk(param, g);
    (void)hipGetLastError();
    if (g) {
        auto it = g_packs.find(g);
        if (it != g_packs.end()) {
            hipStream_t s = it->second->stream;
            if (s) {
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {      // failed inside a capture
                    hipGraph_t gr = nullptr;
                    (void)hipStreamEndCapture(s, &gr);
                    if (gr) (void)hipGraphDestroy(gr);
                }
                (void)hipStreamSynchronize(s);           // whatever was enqueued before the failure
                (void)hipGetLastError();
            }
            it->second->release(); g_packs.erase(it);
        }
    }
    if (param) {
        drop_shard_state(param);
        auto it = g_ctx.find(param);
        aprilsam_amd_stats_t st{};
        if (it != g_ctx.end()) { st = it->second->st; it->second->release(); }
        auto fresh = std::make_unique<Context>();
        fresh->st = st; fresh->st.error_code = code; fresh->st.not_spd = 0;
        g_ctx.put(param, std::move(fresh));
    }
}
template <class Fn> static void guarded(const april_graph_cholesky_param_t *param, const april_graph_t *g, Fn &&fn) {
    try { fn(); }
    catch (const SolverError &e) { on_failure(param, g, e.code, e.msg); }
    catch (const std::bad_alloc &) { on_failure(param, g, ERR_OOM, "host memory exhausted (std::bad_alloc)"); }
    catch (const std::exception &e) { on_failure(param, g, ERR_INTERNAL, e.what()); }
}
template <class Fn> static int guarded_rc(const april_graph_cholesky_param_t *param, const april_graph_t *g, Fn &&fn) {
    try { return fn(); }
    catch (const SolverError &e) { on_failure(param, g, e.code, e.msg); return e.code; }
    catch (const std::bad_alloc &) { on_failure(param, g, ERR_OOM, "host memory exhausted (std::bad_alloc)"); return ERR_OOM; }
    catch (const std::exception &e) { on_failure(param, g, ERR_INTERNAL, e.what()); return ERR_INTERNAL; }
}

// The step counter behind the dependency flags (kernels.hip.h wait_flag) starts here and is advanced once per numeric phase by the phase's
// first kernel.  It is a 32-bit word: a context that has enqueued 2^30 phases (days of back-to-back iterations) starts it over, behind a
// stream synchronisation and with every flag and mark zeroed again (rewind_epoch, called where phases are enqueued).
static const int FIRST_EPOCH = 1 << 20;
struct Context;
static void rewind_epoch(Context &c, hipStream_t s, long long phases);
static void set_const_granules(Context &c, hipStream_t s);
// marginal covariances (solver_marginals.inc.h): what a successful solver call left in the front pool
enum { FACT_NONE = 0, FACT_PLAN = 1, FACT_EXTENDED = 2 };      // no factor / the factor of c.plan / tail fronts appended by the incremental path
static void record_factor(Context &c, int kind, GraphPack &gp);
// what every consumer of the retained factor asks first: is the front pool still what the last successful solver call
// on this param left there?  No after a failed call, LM / GNC / chordal (have_fact, fact_kind), after a phase that moved the step counter
// on (fact_epoch), after a re-plan that no factorisation followed (upload_plan), and while a resident loop is open
static bool no_retained_factor(const Context &c) {
    return !c.have_fact || c.st.not_spd || c.fact_kind == FACT_NONE || c.fact_epoch != c.epoch_steps || c.resident_open;
}
// slack reserved at plan upload so that the incremental path can append without reallocating device buffers
constexpr int INC_NODES = 4096, INC_FACT = 16384, INC_I32 = 4 << 20, INC_DEST = 1 << 20, INC_CHILD = 1 << 18, INC_TAB = 1 << 20;
#define TAIL_POSES (g_opt.tail_poses)         // own poses per tail front of the incremental path (inc_fast_step), option tail_poses (>= 8)
constexpr int MAX_TAIL_FRONTS = INC_NODES / 8 + 8;
constexpr long long INC_POOL_MIN = 8ll << 20;             // doubles (64 MB; the M3500 demo appends ~25 MB of regenerated fronts between two batch steps)

// waves of a k_front_small workgroup (option small_threads)
static int waves_of(int nt) { return nt >= 1024 ? 16 : (nt >= 512 ? 8 : 4); }
// workgroup size of k_front_small on a level with n fronts: latency levels take the big workgroup (more lanes on one
// front's critical path), throughput levels the smaller one (more workgroups per CU)
static long long g_incfail[32] = { 0 };        // APRILSAM_AMD_INC_PROFILE: why inc_fast_step handed a step to a full re-plan (exit number in source order)
static thread_local int g_incfail_last = 0;    // the exit the calling thread's last inc_fast_step left by (aprilsam_amd_debug_inc_forms; 0: it did not fail, or was not tried)
static bool inc_fail(int why) { g_incfail[why & 31]++; g_incfail_last = why; return false; }
static long long g_updstat[6] = { 0 };      // APRILSAM_AMD_INC_PROFILE: general-path steps with / without updated fronts, fronts updated / re-factorised in the former, re-factorised in the latter, steps through k_inc_one
static double g_incsub[8] = { 0 }; static long long g_incsub_n = 0;      // APRILSAM_AMD_INC_PROFILE: host sub-phases of the general incremental path (ms, summed)
static const bool g_incprof_stamps = [] { const char *e = getenv("APRILSAM_AMD_INC_PROFILE"); return e && *e == '2'; }();      // (see IncProf)
static int small_threads_for(size_t n_fronts) { return (int)n_fronts >= g_opt.tp_fronts ? std::min(g_opt.small_threads, g_opt.tp_threads) : g_opt.small_threads; }

// doubles of d_diag a level needs: four NB x NB inverse blocks per active front (the fronts that keep none of their own, FrontDesc::dinv0)
static size_t diag_doubles(int n_big) { return (size_t)std::max(n_big, 1) * OBP * NB * NB; }
// classify the fronts of one level (small / big) and append their launch tables to `tab`
constexpr int BSB_MAX_WGS = 64;               // chain + helper workgroups of one k_backsolve_blk launch (they must be resident together)
template <class Dims, class KeepInv>
static void build_level(LevelPlan &L, std::vector<int> &fronts, std::vector<int> &tab, Dims dims, KeepInv keep_inv) {
    const size_t small_max = (size_t)g_opt.small_lds_kb * 1024;
    L = LevelPlan();
    std::vector<int> small, big;
    size_t maxm = 0;
    auto rows = [&](int t) { int a, b; dims(t, &a, &b); return 3 * (a + b + 1); };
    auto cols = [&](int t) { int a, b; dims(t, &a, &b); return 3 * (a + b); };
    auto nsb_of = [&](int t) { int a, b; dims(t, &a, &b); return a; };
    // throughput levels (far more fronts than compute units): a lower full-LDS limit sends mid-size fronts to panel mode,
    // whose LDS footprint (own columns only) lets several workgroups share a CU
    size_t full_max = small_max;
    if ((int)fronts.size() >= g_opt.tp_fronts && g_opt.tp_lds_kb > 0) full_max = std::min(small_max, (size_t)g_opt.tp_lds_kb * 1024);
    L.full_limit = (long long)full_max;
    L.small_nt = small_threads_for(fronts.size());
    const int nw = waves_of(L.small_nt);
    for (int t : fronts) {
        const int R = rows(t), C = cols(t);
        maxm = std::max<size_t>(maxm, C);
        L.solve_w_lds = std::max(L.solve_w_lds, backsolve_lds(C, 3 * nsb_of(t), true)); L.maxns = std::max(L.maxns, 3 * nsb_of(t));
        const size_t lds_s = small_front_lds(R, C, nw), lds_p = panel_front_lds(R, 3 * nsb_of(t), nw);
        if (lds_s <= full_max) { small.push_back(t); L.small_lds = std::max(L.small_lds, lds_s); }
        else if (g_opt.panel_mode && lds_p <= small_max) { small.push_back(t); L.small_lds = std::max(L.small_lds, lds_p); }   // k_front_small, panel mode
        else if (lds_s <= small_max) { small.push_back(t); L.small_lds = std::max(L.small_lds, lds_s); L.full_limit = std::max(L.full_limit, (long long)lds_s); }
        else big.push_back(t);
    }
    // longest-processing-time first: the widest fronts of a level start first
    std::sort(small.begin(), small.end(), [&](int a, int b) { int ra = rows(a), rb = rows(b); return ra != rb ? ra > rb : a < b; });
    L.all_off = (int)tab.size(); L.n_all = (int)fronts.size();
    tab.insert(tab.end(), fronts.begin(), fronts.end());
    {   // back substitution: fronts with a large update block get their update-row product from k_backsolve_gemv
        std::vector<int> sp;
        for (int t : fronts) { int a, b; dims(t, &a, &b); if (bs_split_front(a, b)) sp.push_back(t); }
        L.bs_gemv = Launch{ (int)tab.size(), 0, (int)sp.size(), 0, false };
        tab.insert(tab.end(), sp.begin(), sp.end());
        L.bs_gemv.pre_off = (int)tab.size();
        int acc = 0; tab.push_back(0);
        for (int t : sp) { acc += (3 * nsb_of(t) + NB - 1) / NB; tab.push_back(acc); }
        L.bs_gemv.grid = acc;
    }
    L.solve_lds = (maxm + NB + 8 + NB * (NB + 1)) * 8;
    L.small_off = (int)tab.size(); L.n_small = (int)small.size();
    tab.insert(tab.end(), small.begin(), small.end());
    L.n_big = (int)big.size();
    if (big.empty()) return;
    std::sort(big.begin(), big.end(), [&](int a, int b) { return nsb_of(a) != nsb_of(b) ? nsb_of(a) > nsb_of(b) : a < b; });
    int list_off = (int)tab.size();
    tab.insert(tab.end(), big.begin(), big.end());
    auto make = [&](int nact, auto count) {
        Launch La; La.list_off = list_off; La.n = nact; La.pre_off = (int)tab.size();
        int acc = 0; tab.push_back(0);
        for (int i = 0; i < nact; i++) { acc += count(big[i]); tab.push_back(acc); }
        La.grid = acc; La.single = acc == nact;
        return La;
    };
    L.asm_big = make((int)big.size(), [&](int t) { return asm_chunks(cols(t) / 3); });
    {   // back substitution of the multi-workgroup fronts 128 columns at a time (k_backsolve_blk): fronts whose inverse
        // diagonal blocks are kept (keep_inv) and whose update-row product comes from k_backsolve_gemv (or is empty);
        // the whole level or nothing: chains + helpers must fit BSB_MAX_WGS workgroups
        std::vector<int> wide, rest, bigs(big);
        std::sort(bigs.begin(), bigs.end());
        int wgs = 0;
        for (int t : fronts) {
            int a, b; dims(t, &a, &b);
            const bool isbig = std::binary_search(bigs.begin(), bigs.end(), t);
            if (isbig && 3 * a <= BSB_FAR && (b == 0 || bs_split_front(a, b)) && keep_inv(t)) { wide.push_back(t); wgs += 1 + bsb_helpers(3 * a); }
            else rest.push_back(t);
        }
        if (!wide.empty() && wgs <= BSB_MAX_WGS && g_opt.blk_backsolve) {
            const int lo = (int)tab.size();
            tab.insert(tab.end(), wide.begin(), wide.end());
            L.bs_blk = Launch{ lo, (int)tab.size(), (int)wide.size(), 0, false };
            int acc = 0; tab.push_back(0);
            for (int t : wide) { acc += 1 + bsb_helpers(3 * nsb_of(t)); tab.push_back(acc); L.bs_blk_lds = std::max(L.bs_blk_lds, bsb_lds(3 * nsb_of(t))); }
            L.bs_blk.grid = acc;
            L.rest_off = (int)tab.size(); L.n_rest = (int)rest.size();
            tab.insert(tab.end(), rest.begin(), rest.end());
            size_t mm = 0; for (int t : rest) mm = std::max<size_t>(mm, cols(t));
            L.rest_lds = (mm + NB + 8 + NB * (NB + 1)) * 8;
        }
    }
    const int steps = (3 * nsb_of(big[0]) + NB - 1) / NB;
    auto active = [&](int sidx) { int nact = 0; while (nact < (int)big.size() && 3 * nsb_of(big[nact]) > sidx * NB) nact++; return nact; };
    // the wide update that closes every outer block of OBP panels (K = the block's columns, everything to its right) -- or, on levels
    // whose wide updates are large (option syrk_pair_tiles), every PAIR of outer blocks (syrk_range)
    const int nobs = (steps + OBP - 1) / OBP;
    auto make_sub = [&](int i0, int i1, auto count) {          // like make() for the fronts big[i0 .. i1)
        Launch La; La.list_off = list_off + i0; La.n = i1 - i0; La.pre_off = (int)tab.size();
        int acc = 0; tab.push_back(0);
        for (int i = i0; i < i1; i++) { acc += count(big[i]); tab.push_back(acc); }
        La.grid = acc; La.single = acc == La.n;
        return La;
    };
    auto tile_for = [&](int i0, int i1, int s_lo, int s_hi, bool ahead) {
        int tile = TILE;
        if (g_opt.syrk_small_tiles > 0) {         // few tiles: 32 x 32 ones (k_syrk_big32)
            long long nt64 = 0;
            for (int i = i0; i < i1; i++) nt64 += syrk_tiles(rows(big[i]), cols(big[i]), 3 * nsb_of(big[i]), s_lo, s_hi, TILE, ahead);
            if (nt64 < g_opt.syrk_small_tiles) tile = TILE / 2;
        }
        return tile;
    };
    {
        long long nt0 = 0;
        for (int i = 0; i < active(0); i++) nt0 += syrk_tiles(rows(big[i]), cols(big[i]), 3 * nsb_of(big[i]), 0, OBP, TILE);
        L.paired = g_opt.syrk_pair_tiles > 0 && nobs >= 2 && nt0 >= g_opt.syrk_pair_tiles;
    }
    for (int o = 0; o < nobs; o++) {
        const int s_lo = o * OBP, s_hi = std::min(s_lo + OBP, steps), nact = active(s_lo);
        if (!L.paired) {
            const int tile = tile_for(0, nact, s_lo, s_hi, false);
            L.syrkw.push_back(make(nact, [&](int t) { return syrk_tiles(rows(t), cols(t), 3 * nsb_of(t), s_lo, s_hi, tile); }));
            L.syrkw.back().tile = tile;
            continue;
        }
        const int G = std::max(2, g_opt.syrk_group), p_lo = (o - o % G) * OBP;       // K = the blocks of the group so far
        if (o % G != G - 1) {
            // not the last block of its group: fronts with a next block (a prefix of `big`, sorted by own columns) update that block's
            // columns only; fronts whose last block this is get their wide update now
            const int n2 = o + 1 < nobs ? active((o + 1) * OBP) : 0;
            int tile = tile_for(0, n2, p_lo, s_hi, true);
            L.syrka.push_back(make_sub(0, n2, [&](int t) { return syrk_tiles(rows(t), cols(t), 3 * nsb_of(t), p_lo, s_hi, tile, true); })); L.syrka.back().tile = tile;
            tile = tile_for(n2, nact, p_lo, s_hi, false);
            L.syrk1.push_back(make_sub(n2, nact, [&](int t) { return syrk_tiles(rows(t), cols(t), 3 * nsb_of(t), p_lo, s_hi, tile); })); L.syrk1.back().tile = tile;
            L.syrkw.push_back(Launch{ 0, 0, 0, 0, false });
        } else {
            const int tile = tile_for(0, nact, p_lo, s_hi, false);
            L.syrka.push_back(Launch{ 0, 0, 0, 0, false }); L.syrk1.push_back(Launch{ 0, 0, 0, 0, false });
            L.syrkw.push_back(make(nact, [&](int t) { return syrk_tiles(rows(t), cols(t), 3 * nsb_of(t), p_lo, s_hi, tile); }));
            L.syrkw.back().tile = tile;
        }
    }
    // outer-block panels (kernels.hip.h: k_block_chain / k_block_solve): per 128-column outer block the active fronts (a
    // prefix of `big`, sorted by own columns) and their row tiles below the diagonal block
    for (int o = 0; o * OBP < steps; o++) {
        const int nact = active(o * OBP);
        Launch bc{ list_off, 0, nact, nact, true };
        L.bchain.push_back(bc);
        long long tiles1 = 0;
        for (int i = 0; i < nact; i++) tiles1 += block_tiles(rows(big[i]), 3 * nsb_of(big[i]), o, 1);
        const int rb = tiles1 > 1024 ? 2 : 1;          // many tiles: 32 rows per wave (half the workgroups, each staging the same L11 once)
        L.btile.push_back(make(nact, [&](int t) { return block_tiles(rows(t), 3 * nsb_of(t), o, rb); }));
        L.btile.back().tile = rb;
    }
}

// Per-rank layout of the front pool in a sharded run: a rank keeps the frontal arrays of the fronts it OWNS and, for
// every child of an owned front that lives on another rank, a "ghost" holding only that child's update block
// ((3 cnu + 3) rows x 3 cnu columns: what the parent's extend-add reads, filled from the wire).  off < 0: not present.
struct ShardLayout { std::vector<long long> off; std::vector<char> ghost; long long pool_doubles = 0; };

// upload the symbolic plan and build the per-level launch tables
// per-factor swap byte of the base plan: bit 0 = the off-diagonal block is stored transposed (Plan::fac_swap), bit 1 = Context::wt
static void fill_swap_host(Context &c) {
    const Plan &P = c.plan;
    c.swap_host.assign(P.fac_swap.begin(), P.fac_swap.end());
    if (c.wt_any) for (size_t f = 0; f < c.swap_host.size() && f < c.wt.size(); f++) c.swap_host[f] |= (unsigned char)(c.wt[f] << 1);
}
static void upload_plan(Context &c, hipStream_t s, const ShardLayout *lay = nullptr) {
    const Plan &P = c.plan;
    const bool uprof = getenv("APRILSAM_AMD_PLAN_PROFILE") != nullptr;
    const double u0 = uprof ? now_ms() : 0;
    c.retire_captures();
    c.lambda_N = -1;
    c.release_sel();                          // (Sigma and its tables describe the plan being replaced)
    c.fact_kind = FACT_NONE;                  // (... and so does the retained factor: its fronts are laid out anew.  The call that plans records its own
                                              // factor when it succeeds; a resident loop that plans and ends without a step leaves the param without one)
    // ---- descriptors + index arrays ----------------------------------------------------------------------------
    std::vector<FrontDesc> &fd = c.inc.fd; fd.assign(P.nF, FrontDesc());
    std::vector<ChildRec> ch(std::max<size_t>(1, P.ch_idx.size()));
    for (int t = 0; t < P.nF; t++) {
        FrontDesc &d = fd[t];
        memset(&d, 0, sizeof(d));
        d.off = lay ? std::max<long long>(lay->off[t], 0) : P.f_off[t]; d.nsb = P.f_nsb[t]; d.nub = P.f_nub[t]; d.first = P.f_first[t];
        d.dest_begin = P.dest_front_ptr[t]; d.dest_end = P.dest_front_ptr[t + 1];
        d.ch_begin = P.ch_ptr[t]; d.ch_end = P.ch_ptr[t + 1];
        d.rows_begin = 0; d.parent = P.f_parent[t];      // rows_begin patched below (absolute offset in the int arena)
    }
    for (int t = 0; t < P.nF; t++) {          // the child with the largest update block (k_assemble_big stores it instead of adding it to zeros)
        int best = -1, second = -1;
        for (int k = P.ch_ptr[t]; k < P.ch_ptr[t + 1]; k++) if (P.f_nub[P.ch_idx[k]] > 0 && (best < 0 || P.f_nub[P.ch_idx[k]] > P.f_nub[P.ch_idx[best]])) best = k;
        for (int k = P.ch_ptr[t]; k < P.ch_ptr[t + 1]; k++) if (k != best && P.f_nub[P.ch_idx[k]] > 0 && (second < 0 || P.f_nub[P.ch_idx[k]] > P.f_nub[P.ch_idx[second]])) second = k;
        fd[t].prim1 = best < 0 ? 0 : best - P.ch_ptr[t] + 1; fd[t].prim2 = second < 0 ? 0 : second - P.ch_ptr[t] + 1;
    }
    for (size_t k = 0; k < P.ch_idx.size(); k++) {
        const int cfr = P.ch_idx[k];
        ChildRec &r = ch[k];
        r.cR = P.rows(cfr); r.cnu = P.f_nub[cfr];
        r.uoff = P.f_off[cfr] + (long long)(3 * P.f_nsb[cfr]) * r.cR + 3 * P.f_nsb[cfr];
        if (lay) {
            if (lay->ghost[cfr]) { r.cR = 3 * r.cnu + 3; r.uoff = lay->off[cfr]; }
            else r.uoff = std::max<long long>(lay->off[cfr], 0) + (long long)(3 * P.f_nsb[cfr]) * r.cR + 3 * P.f_nsb[cfr];
        }
        r.rel_begin = 0; r.pad = cfr;                  // rel_begin patched below; pad keeps the child's front id
    }
    const double u1 = uprof ? now_ms() : 0;
    // slack for the incremental path is only reserved once the param has been used incrementally (a 3-node tutorial graph
    // solved in batch mode should not cost hundreds of MB of HBM); the first incremental call then re-plans once
    const bool inc = c.want_inc;
    const int INC_NODES_ = inc ? INC_NODES : 0, INC_FACT_ = inc ? INC_FACT : 0;
    const size_t INC_I32_ = inc ? INC_I32 : 0, INC_DEST_ = inc ? INC_DEST : 0, INC_CHILD_ = inc ? INC_CHILD : 0, INC_TAB_ = inc ? INC_TAB : 0;
    c.inc.cap_nodes = INC_NODES_; c.inc.cap_fact = INC_FACT_;
    std::vector<int> i32;
    auto put32 = [&](const std::vector<int> &v) { size_t o = i32.size(); i32.insert(i32.end(), v.begin(), v.end()); if (v.empty()) i32.push_back(0); return o; };
    size_t o_rows = put32(P.f_rows), o_rel = put32(P.f_rel);
    // the extend-add's owner table, parallel to f_rel: filled below, once the levels know their workgroup widths.  Nobody reads it with asm_balance
    // off or in a sharded layout (no front gets an own_nw there): then it takes no room in the arena
    const bool own_tab = g_opt.asm_balance && !lay && !P.f_rel.empty();
    const size_t o_own = own_tab ? put32(std::vector<int>(P.f_rel.size(), -1)) : 0;
    size_t o_sb = put32(P.slot_blk); i32.resize(i32.size() + (size_t)3 * INC_FACT_, -1);      // room for factors added incrementally
    size_t o_sr = put32(P.slot_rhs); i32.resize(i32.size() + (size_t)2 * INC_FACT_, -1);
    c.inc.i32_used = (long long)i32.size(); c.inc.dest_used = (long long)P.dest.size(); c.inc.child_used = (long long)P.ch_idx.size();
    for (int t = 0; t < P.nF; t++) fd[t].rows_begin = (int)(o_rows + P.f_rows_ptr[t]);
    for (size_t k = 0; k < P.ch_idx.size(); k++) ch[k].rel_begin = (int)(o_rel + P.f_rows_ptr[ch[k].pad]);
    c.d_i32.need(i32.size() + INC_I32_); c.d_fd.need(fd.size() + 1 + (inc ? MAX_TAIL_FRONTS : 0)); c.d_child.need(ch.size() + INC_CHILD_);
    c.d_dest.need(std::max<size_t>(1, P.dest.size()) + INC_DEST_);
    HIPCHECK(hipMemcpyAsync(c.d_i32.p, i32.data(), i32.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(c.d_fd.p, fd.data(), fd.size() * sizeof(FrontDesc), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(c.d_child.p, ch.data(), ch.size() * sizeof(ChildRec), hipMemcpyHostToDevice, s));
    static_assert(sizeof(DestRec) == sizeof(Plan::DestRec), "DestRec layout");
    if (!P.dest.empty()) HIPCHECK(hipMemcpyAsync(c.d_dest.p, P.dest.data(), P.dest.size() * sizeof(DestRec), hipMemcpyHostToDevice, s));
    c.d_lambda.need((size_t)P.N + INC_NODES_);
    DevPlan &d = c.dp;
    d.nF = P.nF;
    d.fd = c.d_fd.p; d.dest = c.d_dest.p; d.child = c.d_child.p;
    d.f_own = nullptr; d.own_lo = 0; d.own_hi = 0;
    if (own_tab) { d.f_own = c.d_i32.p + o_own - o_rel; d.own_lo = (int)o_rel; d.own_hi = (int)(o_rel + P.f_rel.size()); }      // (indexed like f_rel: ChildRec::rel_begin + block)
    d.f_rows = c.d_i32.p; d.f_rel = c.d_i32.p; d.slot_blk = c.d_i32.p + o_sb; d.slot_rhs = c.d_i32.p + o_sr; d.src_idx = c.d_i32.p;
    c.inc.o_rows = (long long)o_rows; c.inc.o_rel = (long long)o_rel;
    d.lambda = c.d_lambda.p;
    d.prof = nullptr; d.prof_mode = 0;
    d.schur_first_nub = std::max(0, g_opt.schur_first);
    d.epoch = nullptr; d.flevel = nullptr; d.l0 = 0; d.marks = nullptr;      // (epoch: below, once the counter exists; flevel / l0 / marks: set in the copies the multi-level launches take)
    if (getenv("APRILSAM_AMD_KPROF")) { c.d_prof.need((size_t)PROF_SLOTS * P.nF); HIPCHECK(hipMemsetAsync(c.d_prof.p, 0, (size_t)8 * PROF_SLOTS * P.nF, s)); d.prof = c.d_prof.p; d.prof_mode = atoi(getenv("APRILSAM_AMD_KPROF")) >= 2 ? atoi(getenv("APRILSAM_AMD_KPROF")) : 1; }
    c.d_swap.need((size_t)P.F + INC_FACT_); c.d_pos.need((size_t)P.N + INC_NODES_);
    fill_swap_host(c);
    HIPCHECK(hipMemcpyAsync(c.d_swap.p, c.swap_host.data(), P.F, hipMemcpyHostToDevice, s));
    c.wt_dirty = false;
    HIPCHECK(hipMemcpyAsync(c.d_pos.p, P.pos.data(), (size_t)P.N * 4, hipMemcpyHostToDevice, s));
    c.d_perm.need((size_t)P.N + INC_NODES_);
    HIPCHECK(hipMemcpyAsync(c.d_perm.p, P.perm.data(), (size_t)P.N * 4, hipMemcpyHostToDevice, s));

    const double u2 = uprof ? now_ms() : 0;
    // ---- launch tables -------------------------------------------------------------------------------------
    std::vector<int> tab;
    c.levels.assign(P.nLevels, LevelPlan());
    for (int l = 0; l < P.nLevels; l++) {
        std::vector<int> fr(P.lev_fronts.begin() + P.lev_ptr[l], P.lev_fronts.begin() + P.lev_ptr[l + 1]);
        build_level(c.levels[l], fr, tab, [&](int t, int *nsb, int *nub) { *nsb = P.f_nsb[t]; *nub = P.f_nub[t]; }, [](int) { return true; });
    }
    // Owners of the extend-add's destination columns (option asm_balance, plan.h: asm_owners): per single-workgroup front, for the workgroup width
    // of its level's launch -- which is the multi-level launches' width wherever they take the level in.  A launch of another width (k_inc_one,
    // k_assemble_big's 256 threads) and a front without a table (multi-workgroup fronts, sharded layouts, fronts the incremental path regenerates
    // or adds) give column b to wave b mod waves, as before.  One wave per column either way: the sums keep their order and their bits.
    if (own_tab) {
        std::vector<int> own(P.f_rel.size(), -1);
        for (int l = 0; l < P.nLevels; l++) {
            const LevelPlan &L = c.levels[l];
            for (int k = 0; k < L.n_small; k++) {
                const int t = tab[L.small_off + k];
                if (P.ch_ptr[t + 1] == P.ch_ptr[t]) continue;
                fd[t].own_nw = waves_of(L.small_nt);
                asm_owners(P.f_nsb[t] + P.f_nub[t], fd[t].own_nw, P.ch_idx.data() + P.ch_ptr[t], P.ch_ptr[t + 1] - P.ch_ptr[t], P.f_rows_ptr.data(), P.f_nub.data(), P.f_rel.data(), own.data());
            }
        }
        HIPCHECK(hipMemcpyAsync(c.d_i32.p + o_own, own.data(), own.size() * 4, hipMemcpyHostToDevice, s));      // (pageable source, like i32 above: staged before the call returns)
    }
    {   // persistent inverse diagonal blocks of the multi-workgroup fronts (k_block_chain leaves them, k_block_solve and
        // k_backsolve_blk use them): whole outer blocks per front
        long long slots = 0;
        for (int t = 0; t < P.nF; t++) fd[t].dinv0 = -1;
        for (int l = 0; l < P.nLevels; l++) {
            const LevelPlan &L = c.levels[l];
            for (int k = 0; k < L.asm_big.n; k++) { const int t = tab[L.asm_big.list_off + k]; fd[t].dinv0 = (int)slots; slots += (long long)OBP * bsb_blocks(3 * P.f_nsb[t]); }
        }
        c.d_dinv.need((size_t)std::max<long long>(slots, 1) * NB * NB);
        HIPCHECK(hipMemcpyAsync(c.d_fd.p, fd.data(), fd.size() * sizeof(FrontDesc), hipMemcpyHostToDevice, s));
        if (!c.d_bsb_flags.p) { c.d_bsb_flags.need((size_t)BSB_MAX_WGS * 2 * BSB_MAXB); HIPCHECK(hipMemsetAsync(c.d_bsb_flags.p, 0, c.d_bsb_flags.cap * 4, s)); c.d_bsb_far.need((size_t)BSB_MAX_WGS * BSB_FAR); }
    }
    for (int l = 0; l < P.nLevels; l++)
        if (c.levels[l].solve_lds > 160 * 1024)       // k_backsolve keeps x over a front's rows in LDS (~19 000 scalar rows)
            fail(ERR_UNSUPPORTED, "a frontal matrix has more rows than the back-substitution kernel can hold in LDS (an unsplittable dense region "
                 "of more than ~6000 poses); this build does not tile the solve of such a front");
    // ---- multi-level launch over the top of the tree (small fronts only, few per level) ------------------------------
    c.persist_l0 = -1;
    if (g_opt.persist && !lay && P.nLevels >= 3) {
        int l0 = P.nLevels, cnt = 0;
        const int nt_top = c.levels[P.nLevels - 1].small_nt;
        for (int l = P.nLevels - 1; l >= 0; l--) {           // (level 0 too when persist_max_fronts allows: small graphs run as one launch per sweep)
            const LevelPlan &L = c.levels[l];
            if (L.n_big > 0 || L.bs_gemv.grid > 0 || L.small_nt != nt_top || L.n_small != L.n_all || cnt + L.n_small > g_opt.persist_max_fronts) break;
            cnt += L.n_small; l0 = l;
        }
        if (P.nLevels - l0 >= 2) {
            c.persist_l0 = l0; c.p_nt = nt_top; c.p_up_lds = 0; c.p_dn_lds = 0; c.p_up_full = 0; c.p_dn_maxns = 0; c.p_dn_maxnu = 0;
            c.p_up_off = (int)tab.size(); c.p_up_n = cnt;
            for (int l = l0; l < P.nLevels; l++) {                     // children before parents: dependencies have lower workgroup ids
                const LevelPlan &L = c.levels[l];
                for (int k = 0; k < L.n_small; k++) tab.push_back(tab[L.small_off + k]);
                c.p_up_lds = std::max(c.p_up_lds, L.small_lds); c.p_up_full = std::max(c.p_up_full, L.full_limit);
                for (int k = 0; k < L.n_all; k++) { const int t = tab[L.all_off + k]; c.p_dn_lds = std::max(c.p_dn_lds, backsolve_lds(P.cols(t), 3 * P.f_nsb[t], true)); c.p_dn_maxns = std::max(c.p_dn_maxns, 3 * P.f_nsb[t]); c.p_dn_maxnu = std::max(c.p_dn_maxnu, P.cols(t) - 3 * P.f_nsb[t]); }
            }
            c.p_dn_off = (int)tab.size(); c.p_dn_n = cnt;
            for (int l = P.nLevels - 1; l >= l0; l--) { const LevelPlan &L = c.levels[l]; for (int k = 0; k < L.n_all; k++) tab.push_back(tab[L.all_off + k]); }
        }
    }
    // The back substitution's launch takes level 0 in as well (option persist_leaves, bit 0) where only the count stopped the walk above it:
    // level 0 holds single-workgroup fronts only, the launch still fits the LDS with them, and every front keeps the kernel it runs today
    // (k_backsolve_w for the launch and for level 0's own launch, or wave_backsolve = 0), so that the result keeps its bits.  The leaves then
    // wait for their parents' granules with their L panel already in LDS instead of behind a kernel boundary.  Their workgroups follow the
    // upper fronts': every parent keeps a lower id.
    c.persist_dn_l0 = c.persist_l0;
    if (c.persist_l0 == 1 && (g_opt.persist_leaves & 1)) {
        const LevelPlan &L0 = c.levels[0];
        const bool small_only = L0.n_big == 0 && L0.bs_gemv.grid == 0 && L0.bs_blk.grid == 0 && L0.n_small == L0.n_all;
        const bool same_kernel = !g_opt.wave_backsolve || (c.p_dn_maxns <= BSW_MAX_NS && L0.n_all < g_opt.tp_fronts && L0.maxns <= BSW_MAX_NS && L0.solve_w_lds <= 80 * 1024);
        size_t lds = c.p_dn_lds; int maxns = c.p_dn_maxns, maxnu = c.p_dn_maxnu;
        for (int k = 0; k < L0.n_all; k++) { const int t = tab[L0.all_off + k]; lds = std::max(lds, backsolve_lds(P.cols(t), 3 * P.f_nsb[t], true)); maxns = std::max(maxns, 3 * P.f_nsb[t]); maxnu = std::max(maxnu, P.cols(t) - 3 * P.f_nsb[t]); }
        if (small_only && same_kernel && lds <= 160 * 1024) {
            c.persist_dn_l0 = 0; c.p_dn_lds = lds; c.p_dn_maxns = maxns; c.p_dn_maxnu = maxnu;
            for (int k = 0; k < L0.n_all; k++) tab.push_back(tab[L0.all_off + k]);
            c.p_dn_n += L0.n_all;
        }
    }
    // The factorisation's launch takes level 0 in as well (option persist_up) under the same condition: only the count stopped the walk above level
    // 0 (small fronts only, the launch's workgroup size), the launch still fits the LDS, and NO front changes form -- the kernel picks full or panel
    // mode per front from the launch's full_limit, so every front's answer under the joined limit must be the one its own level gives, or the
    // result would lose its bits.  The parents then wait for their leaves' flags (DevPlan::l0 = 0) instead of a kernel boundary.
    c.persist_up_l0 = c.persist_l0;
    const size_t up_lds_own = c.p_up_lds;                  // (what the upper fronts' launch asks for alone: xcd_place's cap, so that its lists do not move)
    if (c.persist_l0 == 1 && g_opt.persist_up > 0) {
        const LevelPlan &L0 = c.levels[0];
        const bool small_only = L0.n_big == 0 && L0.bs_gemv.grid == 0 && L0.n_small == L0.n_all && L0.small_nt == c.p_nt;
        const size_t lds = std::max(c.p_up_lds, L0.small_lds);
        const long long full = std::max(c.p_up_full, L0.full_limit);
        bool same_form = true;
        const int nw = waves_of(c.p_nt);
        for (int l = 0; l < P.nLevels && same_form; l++)
            for (int k = 0; k < c.levels[l].n_small && same_form; k++) {
                const int t = tab[c.levels[l].small_off + k];
                const long long fl = (long long)small_front_lds(P.rows(t), P.cols(t), nw);
                same_form = (fl <= c.levels[l].full_limit) == (fl <= full);
            }
        if (small_only && same_form && lds <= 160 * 1024) { c.persist_up_l0 = 0; c.p_up_lds = lds; c.p_up_full = full; }
    }
    const bool up_joined = c.persist_up_l0 < c.persist_l0;
    const bool up_sched = c.persist_up_l0 == 0 && g_opt.persist_up >= 2;      // (graphs that run one launch per sweep anyway get the order too)
    c.x_up_n = c.x_dn_n = c.x_leaf_n = 0;
    c.u_off = c.p_up_off; c.u_n = c.p_up_n; c.u_fronts = c.persist_l0 >= 0 ? c.p_up_n + (up_joined ? c.levels[0].n_small : 0) : 0;
    if (up_joined && !g_opt.xcd_place && !up_sched) {      // level order, nothing placed: level 0's list, then the upper fronts'
        c.u_off = (int)tab.size(); c.u_n = c.u_fronts;
        for (int k = 0; k < c.levels[0].n_small; k++) tab.push_back(tab[c.levels[0].small_off + k]);
        for (int k = 0; k < c.p_up_n; k++) tab.push_back(tab[c.p_up_off + k]);
    }
    if (c.persist_l0 >= 0 && (g_opt.xcd_place || up_sched)) {
        // XCD-placed copies of the multi-level lists (plan.h: xcd_place), and of level 0's when it is the one launch below them and holds
        // small fronts only (the kernels that may run it return at once on an empty slot).  Classes hold what an XCD runs at once: its
        // compute units times the workgroups per unit the launch's LDS allows.
        int cus = 0;
        HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, physical_device(t_slot)));
        const int per_xcd = std::max(1, cus / 8);
        auto per_cu = [](size_t lds, int nt) { return std::max(1, std::min(2048 / std::max(nt, 64), (int)((160 * 1024) / std::max<size_t>(lds, 1)))); };
        const std::vector<int> up(tab.begin() + c.p_up_off, tab.begin() + c.p_up_off + c.p_up_n);
        const LevelPlan &L0 = c.levels[0];
        const bool leaf = c.persist_l0 == 1 && L0.n_big == 0 && L0.bs_gemv.grid == 0 && L0.bs_blk.grid == 0 && L0.n_small == L0.n_all;
        const std::vector<int> leaves = leaf ? std::vector<int>(tab.begin() + L0.small_off, tab.begin() + L0.small_off + L0.n_small) : std::vector<int>();
        // (leaves: an even share per class, rounded up to whole rounds of the XCD's units -- no class runs more rounds than before)
        const int cap = per_xcd * per_cu(up_lds_own, c.p_nt), cap_leaf = per_xcd * (((int)leaves.size() + 8 * per_xcd - 1) / (8 * per_xcd));
        const XcdLists x = xcd_place(up, leaves, P.f_parent.data(), P.f_nsb.data(), P.nF, cap, cap_leaf);
        if (g_opt.xcd_place) {
            c.x_up_off = (int)tab.size(); c.x_up_n = (int)x.up.size(); tab.insert(tab.end(), x.up.begin(), x.up.end());
            // (level 0 inside the back substitution's launch: its placed list follows the upper fronts' slots there; x.leaf stays the factorisation's)
            const std::vector<int> dn = c.persist_dn_l0 < c.persist_l0 ? dn_with_leaves(x.dn, x.leaf) : x.dn;
            c.x_dn_off = (int)tab.size(); c.x_dn_n = (int)dn.size(); tab.insert(tab.end(), dn.begin(), dn.end());
            c.x_leaf_off = (int)tab.size(); c.x_leaf_n = (int)x.leaf.size(); tab.insert(tab.end(), x.leaf.begin(), x.leaf.end());
            if (!up_joined) { c.u_off = c.x_up_off; c.u_n = c.x_up_n; }
        }
        if (up_joined || up_sched) {
            // the factorisation's one launch: the placed leaf list (whole rounds of 8: every class stays), then the upper fronts' -- level order --
            // or that list in the order of a schedule (plan.h: up_schedule; the slots per class are what the joined launch's LDS allows)
            std::vector<int> list(up_joined ? x.leaf : std::vector<int>());
            list.insert(list.end(), x.up.begin(), x.up.end());
            if (up_sched) list = up_schedule(list, P.f_parent.data(), P.f_nsb.data(), P.nF, per_xcd * per_cu(c.p_up_lds, c.p_nt), g_opt.persist_up);
            c.u_off = (int)tab.size(); c.u_n = (int)list.size(); tab.insert(tab.end(), list.begin(), list.end());
        }
    }
    // (dependency flags / front levels: also used by the extended-plan batch step, whose tail fronts get levels of their own)
    {
        // No flag is ever reset: a finished front publishes the step number, which only grows (a flag that is read late or stale can then only
        // mean "not yet").  New flag memory must therefore start BELOW every step number: zeroed whenever the buffer was (re)allocated --
        // judged by DBuf::need itself, not by the pointer (hipFree + hipMalloc may hand the same address back for the larger block: round-5
        // advisor finding) -- and the counter starts once per context, far above zero.
        const size_t stride = (size_t)P.nF + MAX_TAIL_FRONTS;
        const bool fresh = c.d_flags.need(3 * stride);            // done / x done / vectors ready
        c.d_flevel.need(stride);
        if (fresh || (size_t)c.flag_stride != stride) HIPCHECK(hipMemsetAsync(c.d_flags.p, 0, c.d_flags.cap * 4, s));
        c.flag_stride = (int)stride;
        if (c.d_marks.need(stride)) HIPCHECK(hipMemsetAsync(c.d_marks.p, 0, c.d_marks.cap * 4, s));
        if (c.d_epoch.need(1)) { HIPCHECK(hipMemcpyAsync(c.d_epoch.p, &FIRST_EPOCH, 4, hipMemcpyHostToDevice, s)); c.epoch_steps = 0; }
        d.epoch = c.d_epoch.p;
    }
    if (inc) { c.d_upd.need((size_t)g_opt.persist_max_fronts + 64); c.d_wbuf.need((size_t)1 << 19); }
    HIPCHECK(hipMemcpyAsync(c.d_flevel.p, P.f_level.data(), (size_t)P.nF * 4, hipMemcpyHostToDevice, s));
    if (tab.empty()) tab.push_back(0);
    c.d_tab.need(tab.size() + INC_TAB_);
    c.inc.tab_used = (long long)tab.size();
    c.base_tab = tab;
    const double u3 = uprof ? now_ms() : 0;
    HIPCHECK(hipMemcpyAsync(c.d_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));      // host vectors above go out of scope
    const double u4 = uprof ? now_ms() : 0;

    const long long pool_slack = inc ? std::max<long long>(INC_POOL_MIN, P.pool_doubles / 4) : 0;
    const long long pool_doubles = lay ? lay->pool_doubles : P.pool_doubles;
    c.d_pool.need((size_t)std::max<long long>(pool_doubles, 1) + (size_t)pool_slack);
    c.inc.pool_used = pool_doubles; c.inc.pool_cap = (long long)c.d_pool.cap;
    c.n_guard = 0;
    if (g_opt.pool_guard > 0 && !lay) {
        const long long G = ((long long)g_opt.pool_guard + 31) & ~31ll;
        std::vector<long long> go((size_t)P.nF);
        for (int t = 0; t < P.nF; t++) go[t] = P.f_off[t] + ((((long long)P.rows(t) * P.cols(t)) + 31) & ~31ll);
        c.d_guard.need((size_t)P.nF); c.d_guard_cnt.need(2);
        HIPCHECK(hipMemcpyAsync(c.d_guard.p, go.data(), go.size() * 8, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemsetAsync(c.d_guard_cnt.p, 0, 8, s));
        c.n_guard = P.nF; c.guard_len = (int)G;
        hipLaunchKernelGGL(k_guard, dim3(c.n_guard), dim3(TPB), 0, s, 0, c.d_guard.p, c.n_guard, c.guard_len, c.d_pool.p, c.d_guard_cnt.p);
        HIPCHECK(hipStreamSynchronize(s));      // (go goes out of scope)
    }
    c.d_H.need((size_t)9 * ((size_t)std::max(1, P.n_slots) + (size_t)5 * INC_FACT_)); c.d_x.need((size_t)3 * ((size_t)P.N + INC_NODES_ + 1));
    c.inc.zpos = P.N + INC_NODES_;
    HIPCHECK(hipMemsetAsync(c.d_x.p + (size_t)3 * c.inc.zpos, 0, 24, s));
    {   // The form in which the multi-level back substitutions of this plan hand x over (option tagged_x: 1 granules, 0 write-through x and a
        // flag, 2 the write-back hand-over of every other flag); launch_xmode has the last word per launch.  The granule mirror of x exists only
        // where the option asks for it and such a launch can exist (the batch step's, or an incremental step's later on), and is zeroed with
        // every plan: step numbers of THIS context's counter only grow, so the tags an earlier plan left behind would be older than any step to
        // come -- but its CONSTANT granules (tag XG_CONST at ITS zpos) are not: in a larger plan that position belongs to a pose, and a child
        // would take the zero for its value.  The granules are addressed with 32-bit byte offsets: a system too large for them takes the
        // form every other flag uses.
        const size_t nx = (size_t)3 * ((size_t)P.N + INC_NODES_ + 1);
        const bool mirror = g_opt.tagged_x == 1 && (c.persist_l0 >= 0 || inc) && nx * sizeof(uint4) < ((size_t)1 << 32);
        c.dp.xmode = mirror ? X_TAGGED : g_opt.tagged_x == 0 ? X_WT : X_FLUSH;
        c.dp.xg = nullptr; c.dp.xg_bytes = 0;
        if (mirror) {
            c.d_xg.need(nx);
            HIPCHECK(hipMemsetAsync(c.d_xg.p, 0, c.d_xg.cap * sizeof(uint4), s));
            set_const_granules(c, s);
            c.dp.xg = c.d_xg.p; c.dp.xg_bytes = (unsigned)(nx * sizeof(uint4));
        }
    }
    c.inc.slots_used = P.n_slots;
    c.inc.ready = false; c.inc.t_first.clear(); c.same_topo_batches = 0;
    c.d_bad.need(4); c.h_bad.need(4);
    {   // (a param that is used incrementally: fronts near the root collect the rows of every loop closure since the plan was made and
        // may outgrow the single-workgroup kernel -- room for a few of them on the multi-workgroup path, whose scratch a plan without
        // such fronts would not have; measured on the M3500 demo: 13 steps re-planned for 70 KB of scratch)
        size_t mx = inc ? diag_doubles(160) : 1;          // (incremental steps: room for the big fronts of a regenerated level; a step that needs more re-plans, inc_fail(11))
        for (int l = 0; l < P.nLevels; l++) mx = std::max(mx, diag_doubles(c.levels[l].n_big));
        c.d_diag.need(mx);
    }
    if (uprof) fprintf(stderr, "aprilsam_amd upload: graphs destroyed + descriptors %.3f, index arrays + copies %.3f, launch tables %.3f, last copies + sync %.3f, pools %.3f ms\n", u1 - u0, u2 - u1, u3 - u2, u4 - u3, now_ms() - u4);
    c.st.n_fronts = P.nF; c.st.n_levels = P.nLevels; c.st.max_front_rows = P.max_rows;
    c.st.dn_launch_fronts = c.persist_l0 >= 0 ? c.p_dn_n : 0;       // fronts of the batch step's multi-level back substitution (an incremental step overwrites it with its own)
    c.st.up_launch_fronts = c.u_fronts;                             // ... and of its multi-level factorisation (level 0 included where option persist_up joined it)
    c.st.nnz_L = P.nnzL; c.st.flops_factor = P.flops; c.st.bytes_fronts = 8.0 * (double)pool_doubles;
}

// the x entries that stay zero for good (inc.zpos: what phantom rows point at) are valid in every step
static void set_const_granules(Context &c, hipStream_t s) {
    static const unsigned G[12] = { 0u, (unsigned)XG_CONST, 0u, (unsigned)XG_CONST, 0u, (unsigned)XG_CONST, 0u, (unsigned)XG_CONST, 0u, (unsigned)XG_CONST, 0u, (unsigned)XG_CONST };
    HIPCHECK(hipMemcpyAsync(c.d_xg.p + (size_t)3 * c.inc.zpos, G, sizeof(G), hipMemcpyHostToDevice, s));
}
static void rewind_epoch(Context &c, hipStream_t s, long long phases) {
    c.epoch_steps += phases;
    if (c.epoch_steps < (1ll << 30) || !c.d_epoch.p) return;
    c.fact_kind = FACT_NONE;                                // (marginals: the counter the factor was stamped with starts over)
    HIPCHECK(hipStreamSynchronize(s));                      // nothing in flight reads a flag
    HIPCHECK(hipMemsetAsync(c.d_flags.p, 0, c.d_flags.cap * 4, s));
    HIPCHECK(hipMemsetAsync(c.d_marks.p, 0, c.d_marks.cap * 4, s));
    if (c.d_xg.p) { HIPCHECK(hipMemsetAsync(c.d_xg.p, 0, c.d_xg.cap * sizeof(uint4), s)); set_const_granules(c, s); }      // (tags are step numbers too)
    HIPCHECK(hipMemcpyAsync(c.d_epoch.p, &FIRST_EPOCH, 4, hipMemcpyHostToDevice, s));
    c.epoch_steps = phases;
}

// Options are baked into the launch tables at plan time (build_level: small / panel / big classification, tile counts,
// diagonal-block slots) AND read again when the kernels are enqueued or captured into a hipGraph.  Every change of an option
// that touches either (api_set_option bumps g_opt_epoch) therefore forces a re-plan and a re-capture on every param.
static long long g_opt_epoch = 0;
static long long launch_table_key() { return g_opt_epoch; }
// Batch-like calls, BEFORE prepare_plan: (re)derive Context::wt from the reference's own elimination order of the packed graph
// (refmodel.cpp restates it, aprilsam.c:999-1249) when the graph holds factors with an asymmetric W.  Graphs without such factors -- every
// graph the reference ships or generates -- pay one integer comparison.  Returns true when it ran the model (c.model then describes this
// batch step: the caller need not compute it again).
static void set_wt_any(Context &c, bool v) { c.wt_any = v; }
static bool orient_asymmetric(Context &c, GraphPack &gp) {
    if (gp.n_asym == 0) {
        if (c.wt_any) { c.wt.clear(); set_wt_any(c, false); c.wt_dirty = true; c.wt_serial = -1; }
        return false;
    }
    if (!gp.host_idx.empty()) fail(ERR_UNSUPPORTED, "factors with an asymmetric information matrix next to factors of foreign types: the reference's result depends on its elimination "
                                                    "order here (aprilsam.c:171), which this library only models for xyt / xytpos graphs");
    if (c.wt_serial == gp.serial && c.wt_topo == gp.topo_version && c.wt_content == gp.content_version && (int)c.wt.size() == gp.F) return false;
    const int N = gp.N, F = gp.F;
    c.model.batch(N, F, gp.h_fa.p, gp.h_fb.p);
    c.wt.assign((size_t)F, 0);
    bool any = false;
    for (int f = 0; f < F; f++) {
        const int a = gp.h_fa.p[f], b = gp.h_fb.p[f];
        if (gp.asym[f] && b >= 0 && c.model.pos[b] < c.model.pos[a]) { c.wt[f] = 1; any = true; }
    }
    set_wt_any(c, any);
    c.wt_serial = gp.serial; c.wt_topo = gp.topo_version; c.wt_content = gp.content_version; c.wt_dirty = true;
    return true;
}
// ... and AFTER it: the swap bytes of a REUSED plan follow a changed orientation (a fresh upload carries them already)
static void flush_orientation(Context &c, hipStream_t s) {
    if (!c.wt_dirty || !c.have_plan || !c.d_swap.p) return;
    fill_swap_host(c);
    HIPCHECK(hipMemcpyAsync(c.d_swap.p, c.swap_host.data(), c.swap_host.size(), hipMemcpyHostToDevice, s));
    c.wt_dirty = false;
}
// make sure plan / device buffers match the packed graph; returns true if the plan was reused
// xy_hint = false (chordal initialisation: its result must not depend on the incoming states): a new plan is made from the graph alone
static bool prepare_plan(Context &c, GraphPack &gp, const april_graph_t *g, bool upload = true, bool xy_hint = true) {
    const int N = gp.N, F = gp.F;
    bool same = c.have_plan && c.patN == N && (int)c.pat.size() == 2 * F && c.plan.leaf_nodes == g_opt.leaf_nodes && c.plan_pin == g_opt.pin_last &&
                c.plan_persist == launch_table_key() && c.inc.t_first.empty();        // (a plan extended by tail fronts is only driven by inc_fast_step)
    if (same && !(c.pat_serial == gp.serial && c.pat_topo == gp.topo_version)) {      // (same pack, endpoints untouched since the last comparison: nothing to compare)
        for (int i = 0; i < F && same; i++) same = c.pat[2 * i] == gp.h_fa.p[i] && c.pat[2 * i + 1] == gp.h_fb.p[i];
    }
    c.pat_serial = gp.serial; c.pat_topo = gp.topo_version;       // (c.pat equals the packed endpoints from here on, either way)
    if (same) return true;
    c.pat.resize((size_t)2 * F);
    for (int i = 0; i < F; i++) { c.pat[2 * i] = gp.h_fa.p[i]; c.pat[2 * i + 1] = gp.h_fb.p[i]; }
    c.patN = N; c.plan_pin = g_opt.pin_last; c.plan_persist = launch_table_key();
    std::vector<double> xy((size_t)2 * N);
    for (int i = 0; i < N; i++) { xy[2 * i] = gp.h_state.p[3 * i]; xy[2 * i + 1] = gp.h_state.p[3 * i + 1]; }
    const double tb0 = now_ms();
    build_plan(c.plan, N, F, c.pat.data(), xy_hint ? xy.data() : nullptr, g_opt.leaf_nodes);
    if (g_opt.pool_guard > 0) {              // debug: a guard band behind every frontal array (upload_plan fills them, check_guard reads them)
        Plan &P = c.plan;
        const long long G = ((long long)g_opt.pool_guard + 31) & ~31ll;
        long long off = 0;
        for (int t = 0; t < P.nF; t++) { P.f_off[t] = off; off += ((((long long)P.rows(t) * P.cols(t)) + 31) & ~31ll) + G; }
        P.pool_doubles = off;
    }
    const double tb1 = now_ms();
    if (upload) upload_plan(c, gp.stream);
    if (getenv("APRILSAM_AMD_PLAN_PROFILE")) fprintf(stderr, "aprilsam_amd plan: N=%d build %.3f ms upload %.3f ms\n", N, tb1 - tb0, now_ms() - tb1);
    c.have_plan = true;
    return false;
}

