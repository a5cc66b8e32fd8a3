// solver_launch.inc.h -- part of solver.hip.cpp (ONE translation unit), included from there after solver_context.inc.h, inside namespace asam.
// Contents: the launch layer -- ONE launcher per templated kernel family (every instantiation and its attribute call are listed here and
// nowhere else), the launches of one level, the numeric phase of a batch step (enqueue_numeric) and its replay as a captured hipGraph.

template <class K> static void allow_full_lds(K kern) { HIPCHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); }
static void set_small_attr() {
    static std::once_flag once[MAX_SLOTS];          // (function attributes are kept per device)
    std::call_once(once[physical_device(t_slot) % MAX_SLOTS], [] {
        allow_full_lds(k_front_small<256>); allow_full_lds(k_front_small<512>); allow_full_lds(k_front_small<1024>);
        allow_full_lds(k_backsolve_t<false>); allow_full_lds(k_backsolve_t<true>); allow_full_lds(k_backsolve_w); allow_full_lds(k_backsolve_t<false, true>);
        allow_full_lds(k_block_chain); allow_full_lds(k_backsolve_blk); allow_full_lds(k_block_solve<1>); allow_full_lds(k_block_solve<2>);
        allow_full_lds(k_inc_one<256>); allow_full_lds(k_inc_one<512>); allow_full_lds(k_inc_one<1024>);
    });
}
// k_front_small with nt threads per workgroup (option small_threads: 256 / 512 / 1024); `a`: the kernel's arguments, with or without the trailing UpdCtx
template <class... Args> static void launch_front_small_nt(int nt, int grid, size_t lds, hipStream_t s, const Args &...a) {
    if (nt >= 1024) hipLaunchKernelGGL(k_front_small<1024>, dim3(grid), dim3(1024), lds, s, a...);
    else if (nt >= 512) hipLaunchKernelGGL(k_front_small<512>, dim3(grid), dim3(512), lds, s, a...);
    else hipLaunchKernelGGL(k_front_small<256>, dim3(grid), dim3(256), lds, s, a...);
}
// k_inc_one, one workgroup of nt threads (option inc_one_threads); `a` as above
template <class... Args> static void launch_inc_one_nt(int nt, size_t lds, hipStream_t s, const Args &...a) {
    if (nt >= 1024) hipLaunchKernelGGL(k_inc_one<1024>, dim3(1), dim3(1024), lds, s, a...);
    else if (nt >= 512) hipLaunchKernelGGL(k_inc_one<512>, dim3(1), dim3(512), lds, s, a...);
    else hipLaunchKernelGGL(k_inc_one<256>, dim3(1), dim3(256), lds, s, a...);
}

// Event pairs around every kernel launch of an instrumented pass (NumericArgs::ktime -> c.k_ev / c.k_ids / c.k_lev; collect_kernel_times
// folds them).  Default-constructed it does nothing: no_timer is what every launch outside such a pass is given (never written).
struct KTimer {
    Context *c = nullptr; hipStream_t s = nullptr; size_t nev = 0;
    int level = -1;                                  // (profile: the level the launches that follow belong to; multi-level launches: their first level)
    void tic(int id) {
        if (!c) return;
        if (c->k_ev.size() < nev + 2) { c->k_ev.resize(nev + 2); HIPCHECK(hipEventCreate(&c->k_ev[nev])); HIPCHECK(hipEventCreate(&c->k_ev[nev + 1])); }
        HIPCHECK(hipEventRecord(c->k_ev[nev], s));
        c->k_ids.push_back(id); c->k_lev.push_back(level);
    }
    void toc() { if (c) { HIPCHECK(hipEventRecord(c->k_ev[nev + 1], s)); nev += 2; } }
};
static KTimer no_timer;

// The back substitution of the `n` fronts of `list`, one workgroup per front, in the form the caller chose: column-per-lane with the L panel in LDS
// (k_backsolve_w; `split` unused), 32 columns at a time (k_backsolve_t), the same for fronts of more than BS_TALL_ROWS rows.  Which form a list
// can take is the caller's question: the predicates differ on purpose (a level of a plan / the few fronts of an incremental step).
enum BsForm { BS_WAVE, BS_THREAD, BS_THREAD_TALL };
static void launch_backsolve_list(Context &c, hipStream_t s, BsForm form, const int *list, int n, size_t lds, int split, int *bad, const UpdArgs &upd) {
    if (form == BS_WAVE) hipLaunchKernelGGL(k_backsolve_w, dim3(n), dim3(TPB), lds, s, c.dp, list, c.d_pool.p, c.d_x.p, (int *)nullptr, bad, upd);
    else if (form == BS_THREAD_TALL) hipLaunchKernelGGL((k_backsolve_t<false, true>), dim3(n), dim3(TPB), lds, s, c.dp, list, c.d_pool.p, c.d_x.p, split, (int *)nullptr, 0, bad, upd);
    else hipLaunchKernelGGL((k_backsolve_t<false>), dim3(n), dim3(TPB), lds, s, c.dp, list, c.d_pool.p, c.d_x.p, split, (int *)nullptr, 0, bad, upd);
}

// The form of a level's one-workgroup-per-front launch, whose list asks for solve_lds bytes in the 32-columns-at-a-time form.  Latency-bound
// levels of small fronts: column-per-lane form with the L panel in LDS (at least two workgroups per CU).  (One place for launch_backsolve
// and for what aprilsam_amd_debug_front_forms reports.)
static BsForm level_bs_form(const LevelPlan &L, size_t solve_lds) {
    const bool wave = g_opt.wave_backsolve && L.bs_gemv.grid == 0 && L.n_all < g_opt.tp_fronts && L.maxns <= BSW_MAX_NS && L.solve_w_lds <= 80 * 1024;
    return wave ? BS_WAVE : solve_lds >= (size_t)(BS_TALL_ROWS + NB + 8 + NB * (NB + 1)) * 8 ? BS_THREAD_TALL : BS_THREAD;
}
// ... and of a multi-level back substitution whose widest own part has maxns columns: column-per-lane, or k_backsolve_t waiting on flags
static bool multi_bs_wave(int maxns) { return g_opt.wave_backsolve && maxns <= BSW_MAX_NS; }
// back substitution of one level: update-row products of the large fronts on many workgroups, then one workgroup per front
// (list_off >= 0: the level's list of every front replaced by the list_n entries there -- an XCD-placed list of a level of small fronts only)
static void launch_backsolve(Context &c, const LevelPlan &L, hipStream_t s, KTimer &kt, const int *tab = nullptr, UpdArgs upd = UpdArgs{}, int list_off = -1, int list_n = 0) {
    if (!tab) tab = c.d_tab.p;
    if (!L.n_all) return;
    kt.tic(K_BACKSOLVE);
    if (L.bs_gemv.grid > 0)
        hipLaunchKernelGGL(k_backsolve_gemv, dim3(L.bs_gemv.grid), dim3(TPB), 0, s, c.dp, tab + L.bs_gemv.list_off, tab + L.bs_gemv.pre_off,
                           L.bs_gemv.n, c.d_pool.p, c.d_x.p);
    // wide fronts: chain + helper workgroups (k_backsolve_blk); the level's other fronts below
    int n_all = list_off >= 0 ? list_n : L.n_all, all_off = list_off >= 0 ? list_off : L.all_off; size_t solve_lds = L.solve_lds;
    if (L.bs_blk.grid > 0) {
        hipLaunchKernelGGL(k_backsolve_blk, dim3(L.bs_blk.grid), dim3(TPB), L.bs_blk_lds, s, c.dp, tab + L.bs_blk.list_off, tab + L.bs_blk.pre_off, L.bs_blk.n,
                           c.d_pool.p, c.d_x.p, c.d_dinv.p, c.d_bsb_flags.p, c.d_bsb_far.p, L.bs_gemv.grid > 0 ? 1 : 0, c.d_bad.p, upd);
        n_all = L.n_rest; all_off = L.rest_off; solve_lds = L.rest_lds;
        if (!n_all) { kt.toc(); return; }
    }
    const BsForm form = level_bs_form(L, solve_lds);
    launch_backsolve_list(c, s, form, tab + all_off, n_all, form == BS_WAVE ? L.solve_w_lds : solve_lds, L.bs_gemv.grid > 0 ? 1 : 0, c.d_bad.p, upd);
    kt.toc();
}

// The hand-over form of ONE multi-level back substitution whose tallest update block has max_upd_rows rows: granules are gathered one per lane
// (kernels.hip.h gather_x), so a launch with a taller block takes the form every other flag uses.  (Of the batch plans only a designed one puts such a front
// into a multi-level launch -- a front of 86 update blocks that still fits a workgroup's LDS needs four or more ancestors of at most 24-33 poses
// each: the seven-level clique tree of tests/support/clique_trees.py -- but an incremental step's fronts near the root collect rows without such
// a bound.)
static int launch_xmode(const Context &c, int max_upd_rows) { return c.dp.xmode == X_TAGGED && max_upd_rows > TPB ? (int)X_FLUSH : c.dp.xmode; }
static int device_cus() {
    int cus = 0;
    HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, physical_device(t_slot)));
    return cus;
}
// Dynamic LDS of a multi-level back substitution of `grid` workgroups: two workgroups of more than 80 KB each cannot share a compute unit's 160 KB.
// The write-through form NEEDS one workgroup of the launch per unit (kernels.hip.h publish_flag_wt): it always gets the larger request, and a
// grid of more workgroups than units (persist_max_fronts above its default, the empty slots of a placed list) then runs in rounds of one per
// unit -- deadlock-free as ever by the order of the ids, slower than two per unit.  The granules need no such thing; they get it where it is
// free, on a grid that fits the device (M3500: 216 slots), so that a spinning workgroup does not sit beside a working one.
static size_t handover_lds(int xmode, size_t lds, int grid) {
    if (xmode == X_WT || (xmode == X_TAGGED && grid <= device_cus())) return std::max(lds, HANDOVER_LDS_MIN);
    return lds;
}
// the plan as a step's multi-level launches see it (flags carry the step number): with the hand-over form of a launch whose tallest update block
// has max_upd_rows rows; as the batch path's two launches over the levels >= persist_l0 see it
static DevPlan launch_plan(const Context &c, DevPlan d, int max_upd_rows) { d.xmode = launch_xmode(c, max_upd_rows); return d; }
static DevPlan persist_plan(const Context &c) { DevPlan d = c.dp; d.flevel = c.d_flevel.p; d.l0 = c.persist_l0; d.xmode = launch_xmode(c, c.p_dn_maxnu); return d; }
// The multi-level back substitution: ONE launch over the n fronts of `list` (parents before children), a front waiting on its parent's entry of
// xflags.  dp: the plan with the launch's hand-over form decided (launch_plan / persist_plan); lds / maxns: the list's largest L panel in LDS
// and widest own part.
static void launch_backsolve_multi(Context &c, hipStream_t s, const DevPlan &dp, const int *list, int n, size_t lds, int maxns, int *xflags, const UpdArgs &upd) {
    lds = handover_lds(dp.xmode, lds, n);
    if (multi_bs_wave(maxns)) hipLaunchKernelGGL(k_backsolve_w, dim3(n), dim3(TPB), lds, s, dp, list, c.d_pool.p, c.d_x.p, xflags, c.d_bad.p, upd);
    else hipLaunchKernelGGL((k_backsolve_t<true>), dim3(n), dim3(TPB), lds, s, dp, list, c.d_pool.p, c.d_x.p, 0, xflags, 1, c.d_bad.p, upd);
}

// debug option pool_poison (kernels.hip.h k_poison): NaN into everything the step's launches hand from one workgroup to another
static void enqueue_poison(Context &c, hipStream_t s, const int *list, int n, int what = 3, const UpdRec *recs = nullptr) {
    if (g_opt.pool_poison <= 0 || n <= 0) return;
    static_assert(offsetof(UpdRec, mode) % 4 == 0 && sizeof(UpdRec) % 4 == 0, "UpdRec::mode as a strided int");
    hipLaunchKernelGGL(k_poison, dim3(n), dim3(TPB), 0, s, c.dp, list, n, recs ? (const int *)((const char *)recs + offsetof(UpdRec, mode)) : (const int *)nullptr,
                       (int)(sizeof(UpdRec) / 4), what, c.d_pool.p, c.d_x.p);
}
// the multi-level launch of the factorisation: every small front of levels >= persist_up_l0, in the order upload_plan chose (empty slots included)
static void launch_front_persist(Context &c, hipStream_t s) {
    const int *list = c.d_tab.p + c.u_off, n = c.u_n;
    DevPlan dpe = persist_plan(c);
    dpe.l0 = c.persist_up_l0;                              // (level 0 inside the launch: its parents wait for its flags)
    if (g_opt.skip_flag_waits > 0) dpe.l0 = 1 << 30;       // debug (negative control of pool_poison): no front of this launch waits for its children
    launch_front_small_nt(c.p_nt, n, c.p_up_lds, s, dpe, list, c.d_pool.p, c.d_H.p, c.d_bad.p, c.p_up_full, c.d_flags.p, 1);
}

// the small fronts of one level (list_off >= 0: the list_n entries there instead of the level's own list -- an XCD-placed list)
static void launch_front_small(Context &c, const LevelPlan &L, hipStream_t s, const int *tab = nullptr, int list_off = -1, int list_n = 0) {
    if (!tab) tab = c.d_tab.p;
    const int off = list_off >= 0 ? list_off : L.small_off, n = list_off >= 0 ? list_n : L.n_small;
    launch_front_small_nt(L.small_nt, n, L.small_lds, s, c.dp, tab + off, c.d_pool.p, c.d_H.p, c.d_bad.p, L.full_limit, (int *)nullptr, 0);
}

// The big fronts of one level, 128 columns (an outer block of OBP panels) at a time: diagonal block in LDS with the inverses of its four
// 32 x 32 diagonal blocks as a by-product (k_block_chain), row solves on the matrix cores (k_block_solve), then ONE wide update of
// everything to the right with K = the block's columns (k_syrk_big / k_syrk_big32).
static void enqueue_big_steps(Context &c, const LevelPlan &L, hipStream_t s, KTimer &kt, const int *tab = nullptr) {
    if (!tab) tab = c.d_tab.p;
    const int xcd = std::max(0, g_opt.syrk_xcd_order) << SYRK_MODE_XCD_SHIFT;
    for (size_t o = 0; o < L.bchain.size(); o++) {
        const Launch &bc = L.bchain[o], &bt = L.btile[o], &sw = L.syrkw[o];
        kt.tic(K_PANEL_BIG);
        hipLaunchKernelGGL(k_block_chain, dim3(bc.n), dim3(BCH_THREADS), block_chain_lds(), s, c.dp, tab + bc.list_off, (int)o, c.d_pool.p, c.d_diag.p, c.d_dinv.p, c.d_bad.p);
        if (bt.grid > 0) {
            if (bt.tile == 2) hipLaunchKernelGGL(k_block_solve<2>, dim3(bt.grid), dim3(TPB), block_solve_lds(), s, c.dp, tab + bt.list_off, tab + bt.pre_off, bt.n, (int)o, c.d_pool.p, c.d_diag.p, c.d_dinv.p);
            else hipLaunchKernelGGL(k_block_solve<1>, dim3(bt.grid), dim3(TPB), block_solve_lds(), s, c.dp, tab + bt.list_off, tab + bt.pre_off, bt.n, (int)o, c.d_pool.p, c.d_diag.p, c.d_dinv.p);
        }
        kt.toc();
        auto wide = [&](const Launch &w, int s_lo, int s_hi, int mode) {
            if (w.grid <= 0) return;
            kt.tic(K_SYRK_BIG);
            // (s_lo, s_hi) in panel steps: the kernel clips s_hi * NB to the front's own columns
            if (w.tile == TILE / 2) hipLaunchKernelGGL(k_syrk_big32, dim3(w.grid), dim3(TPB), 0, s, c.dp, tab + w.list_off, tab + w.pre_off, w.n, s_lo, s_hi, mode | xcd, c.d_pool.p);
            else hipLaunchKernelGGL(k_syrk_big, dim3(w.grid), dim3(TPB), 0, s, c.dp, tab + w.list_off, tab + w.pre_off, w.n, s_lo, s_hi, mode | xcd, c.d_pool.p);
            kt.toc();
        };
        const int G = std::max(2, g_opt.syrk_group), g0 = (int)(o - o % G) * OBP;
        if (!L.paired) wide(sw, (int)o * OBP, (int)(o + 1) * OBP, 1);
        else if ((int)(o % G) != G - 1) { wide(L.syrka[o], g0, (int)(o + 1) * OBP, 2); wide(L.syrk1[o], g0, (int)(o + 1) * OBP, 1); }
        else wide(sw, g0, (int)(o + 1) * OBP, 1);
    }
}

// kernels of one level of the factorisation (small LDS fronts, big multi-workgroup path)
static void enqueue_factor_level(Context &c, const LevelPlan &L, hipStream_t s, KTimer &kt, const int *tab = nullptr) {
    if (!tab) tab = c.d_tab.p;
    if (L.n_small) {
        kt.tic(K_FRONT_SMALL);
        launch_front_small(c, L, s, tab);
        kt.toc();
    }
    if (L.n_big) {
        kt.tic(K_ASSEMBLE_BIG);
        hipLaunchKernelGGL(k_assemble_big, dim3(L.asm_big.grid), dim3(TPB), L.asm_lds, s, c.dp, tab + L.asm_big.list_off,
                           tab + L.asm_big.pre_off, L.asm_big.n, c.d_pool.p, c.d_H.p);
        kt.toc();
        enqueue_big_steps(c, L, s, kt, tab);
    }
}

// ---- the factor families: one launcher each, and each family's hooks side by side ----------------------------------------------------
// A family rides on the plain xyt / xytpos slots with up to three hooks, each one launch over the family's table and none for a pack
// without it: what k_linearize_t reads from the slot BEFORE the linearisation, what replaces the contributions it wrote AFTER it, and the
// TERM that replaces the slot's term of the objective.
//   family            table                launcher          before              after              term (CHI2 / LM)
//   max-mixture       gp.d_mx_*            launch_mixture    k_select_mixture    --                 k_chi2_mixture / k_lm_cost_mixture
//   robust            gp.d_rb_*            launch_robust     k_robust_weight     --                 k_chi2_robust / k_lm_cost_robust
//   GNC candidates    gp.d_gc_* (gc_n)     launch_gnc        k_gnc_weight        --                 -- / k_gnc_cost
//   polar             gp.d_pl_*            launch_polar      k_polar_slot        --                 k_chi2_polar (both)
//   dense Gaussian    gp.gauss_tab()       launch_gaussian   --                  k_gaussian_slot    k_chi2_gaussian (both)
// `a` is what follows the table (and, where the kernel takes them, the endpoints fa, fb and the slots' z) in the kernel's arguments.
template <class K, class... Args> static void launch_mixture(hipStream_t s, GraphPack &gp, K kern, const Args &...a) {
    const int M = gp.n_max();
    if (M == 0) return;
    hipLaunchKernelGGL(kern, dim3((M + TPB - 1) / TPB), dim3(TPB), 0, s, M, (const int *)gp.d_mx_f.p, (const int *)gp.d_mx_k.p, (const double *)gp.d_mx_z.p,
                       (const double *)gp.d_mx_W.p, (const double *)gp.d_mx_c.p, (const int *)gp.d_fa.p, (const int *)gp.d_fb.p, a...);
}
template <class K, class... Args> static void launch_robust(hipStream_t s, GraphPack &gp, K kern, const Args &...a) {
    const int R = gp.n_robust();
    if (R == 0) return;
    hipLaunchKernelGGL(kern, dim3((R + TPB - 1) / TPB), dim3(TPB), 0, s, R, (const int *)gp.d_rb_f.p, (const int *)gp.d_rb_kind.p, (const double *)gp.d_rb_c.p,
                       (const double *)gp.d_rb_W0.p, (const int *)gp.d_fa.p, (const int *)gp.d_fb.p, (const double *)gp.d_z.p, a...);
}
// (the candidates of an aprilsam_amd_optimize_gnc run, gp.gc_n of them: the caller asks for gc_n > 0)
template <class K, class... Args> static void launch_gnc(hipStream_t s, GraphPack &gp, K kern, const Args &...a) {
    hipLaunchKernelGGL(kern, dim3((gp.gc_n + TPB - 1) / TPB), dim3(TPB), 0, s, gp.gc_n, (const int *)gp.d_gc_f.p, (const double *)gp.d_gc_W0.p, (const GncPar *)gp.d_gc_par.p, a...);
}
template <class K, class... Args> static void launch_polar(hipStream_t s, GraphPack &gp, K kern, const Args &...a) {
    const int P = gp.n_polar();
    if (P == 0) return;
    hipLaunchKernelGGL(kern, dim3((P + TPB - 1) / TPB), dim3(TPB), 0, s, P, (const int *)gp.d_pl_f.p, (const int *)gp.d_pl_kind.p, (const double *)gp.d_pl_z.p,
                       (const double *)gp.d_pl_W.p, (const int *)gp.d_fa.p, (const int *)gp.d_fb.p, a...);
}
// (one wave per dense Gaussian factor)
template <class K, class... Args> static void launch_gaussian(hipStream_t s, GraphPack &gp, K kern, const Args &...a) {
    const int G = gp.n_gaussian();
    if (G == 0) return;
    hipLaunchKernelGGL(kern, dim3(G), dim3(64), 0, s, gp.gauss_tab(), a...);
}

// BEFORE: every linearisation is preceded by ...
// max factors: the component selected at the l_point into the factor's slot
static void enqueue_select(GraphPack &gp, hipStream_t s) { launch_mixture(s, gp, k_select_mixture, (const double *)gp.d_lp.p, gp.d_z.p, gp.d_W.p, gp.d_sel.p); }
// robust factors: W_eff = w(s) W0 into the factor's slot; upt: the unary factors' points as the linearisation that follows reads them
static void enqueue_robust(GraphPack &gp, hipStream_t s, const double *upt) {
    launch_robust(s, gp, k_robust_weight, (const double *)gp.d_lp.p, (const double *)gp.d_state.p, upt, gp.d_W.p, gp.d_rb_w.p);
}
// GNC candidates: W_eff = w_mu(s) W0 (none outside an aprilsam_amd_optimize_gnc run: gc_n = 0)
static void enqueue_gnc_weight(GraphPack &gp, hipStream_t s, const double *upt) {
    if (gp.gc_n == 0) return;
    launch_gnc(s, gp, k_gnc_weight, (const int *)gp.d_fa.p, (const int *)gp.d_fb.p, (const double *)gp.d_z.p, (const double *)gp.d_lp.p, (const double *)gp.d_state.p, upt, gp.d_W.p, gp.d_gc_w.p);
}
// polar factors: z_eff, W_eff at the l_points (what k_linearize_t reads for a binary factor) into the factor's slot
static void enqueue_polar(GraphPack &gp, hipStream_t s) { launch_polar(s, gp, k_polar_slot, (const double *)gp.d_lp.p, gp.d_z.p, gp.d_W.p); }
static void enqueue_families_before(GraphPack &gp, hipStream_t s, const double *upt) {
    enqueue_select(gp, s);
    enqueue_robust(gp, s, upt);
    enqueue_gnc_weight(gp, s, upt);
    enqueue_polar(gp, s);
}

// The one-wave-per-work-entry kernels of the retained-factor consumers (selinv.hip.h, pathsolve.hip.h, treesolve.hip.h): four waves per
// workgroup over the entries of `sp`, times `column_tiles` in the grid's y (the tree solve's 16-column tiles; 1 elsewhere).  Every such
// kernel starts with (fronts, entries, number of entries); `a` is what follows.  An empty span: no launch
template <class K, class Fr, class E, class... Args>
static void launch_waves(K kern, hipStream_t s, Span sp, unsigned column_tiles, const Fr *fr, const E *ent, const Args &...a) {
    if (sp.n == 0) return;
    hipLaunchKernelGGL(kern, dim3((unsigned)((sp.n + 3) / 4), column_tiles), dim3(TPB), 0, s, fr, ent + sp.off, sp.n, a...);
}

// The kernels of polargate.hip.h, behind the path solves of a gating call: k_gate_polar runs one thread per candidate
// (per_item = false: `work` candidates), k_associate_polar one workgroup per observation (per_item = true: `work` observations); `a` are the
// kernel's arguments.  Nothing to gate: no launch
template <class K, class... Args> static void launch_polar_gate(hipStream_t s, K kern, int work, bool per_item, const Args &...a) {
    if (work <= 0) return;
    hipLaunchKernelGGL(kern, dim3((unsigned)(per_item ? work : (work + PG_T - 1) / PG_T)), dim3(PG_T), 0, s, a...);
}

// The frame of jointgate.hip.h with rider R (JointGate; infomeasure.hip.h's SetLogdet, InfoGain), behind the path solves of a call: one wave
// per list; `a` = what follows the count.  No lists: no launch
template <class R, class... Args> static void launch_block_chol(hipStream_t s, int n_lists, const Args &...a) {
    if (n_lists <= 0) return;
    hipLaunchKernelGGL(k_block_chol<R>, dim3((unsigned)n_lists), dim3(JG_T), 0, s, n_lists, a...);
}

// The kernels of infomeasure.hip.h that read the factor itself: k_logdet_partial (one wave per entry, four per
// workgroup) and k_logdet_sum (one workgroup), which follows it on the stream and is enqueued with it
static void launch_info(hipStream_t s, int n_ent, const LdEnt *ent, const double *pool, double *part, int *nbad, double *out) {
    if (n_ent > 0) hipLaunchKernelGGL(k_logdet_partial, dim3((unsigned)((n_ent + 3) / 4)), dim3(TPB), 0, s, ent, n_ent, pool, part, nbad);
    hipLaunchKernelGGL(k_logdet_sum, dim3(1), dim3(LD_SUM_T), 0, s, n_ent, (const double *)part, (const int *)nbad, out);
}

// The kernel of fixed.hip.h that runs one thread per record of the pack's fixed table and one per fixed node: the
// slots of d_H named by the records become zero, d_lambda at the fixed nodes' positions 1.0.  None for a pack without fixed nodes.  It
// follows whatever wrote the slots and d_lambda for the step and precedes the first assembly kernel, inside every captured graph
static void launch_fixed(hipStream_t s, Context &c, GraphPack &gp) {
    const int NF = gp.n_fixed();
    if (NF == 0) return;
    const int R = (int)gp.fx_rec.size();
    // (the kernel indexes the plan's tables with what the pack holds: both were made from the same packed graph)
    if (gp.fx_dirty || gp.fx_topo != gp.topo_version || gp.fx_nodes.back() >= c.plan.N || (R > 0 && gp.fx_rec.back().x >= c.plan.F))
        fail(ERR_INTERNAL, "fixed table out of step with the plan (%d nodes of %d, %d records, entries < %d)", NF, c.plan.N, R, c.plan.F);
    hipLaunchKernelGGL(k_fix_mask, dim3((R + NF + TPB - 1) / TPB), dim3(TPB), 0, s, R, (const int2 *)gp.d_fx_rec.p, NF, (const int *)gp.d_fx_nodes.p, (const int *)c.d_pos.p,
                       c.dp.slot_blk, c.dp.slot_rhs, c.d_H.p, c.d_lambda.p);
}

// AFTER: every linearisation is followed by the dense Gaussian factors' blocks and rhs segments at the l_points, in place of the zero
// contributions k_linearize_t made of their null slots, and then by the fixed-node mask -- last, after everything that writes a slot
static void enqueue_families_after(Context &c, GraphPack &gp, hipStream_t s) {
    launch_gaussian(s, gp, k_gaussian_slot, (const double *)gp.d_lp.p, (const unsigned char *)c.d_swap.p, c.dp.slot_blk, c.dp.slot_rhs, c.d_H.p);
    launch_fixed(s, c, gp);
}

// TERM: the per-factor terms of the objective at the state array `st` -> terms[0 .. F), under one of two conventions:
// CHI2 is april_graph_chi2's (1/2 on binary xyt terms, a max factor without its c_k), LM the least-squares objective the optimisers
// minimise (no 1/2, min_k of the score, rho_mu for the candidates of a GNC run).  The plain kernel writes every slot's term, then each
// family replaces its own in place, so the sum that follows keeps its order.  The one list of families
enum class Convention { CHI2, LM };
static void enqueue_objective(GraphPack &gp, hipStream_t s, Convention cv, const double *st, double *terms) {
    const int F = gp.F;
    const bool lm = cv == Convention::LM;
    hipLaunchKernelGGL(lm ? k_lm_cost : k_chi2, dim3((F + TPB - 1) / TPB), dim3(TPB), 0, s, F, gp.d_fa.p, gp.d_fb.p, gp.d_z.p, gp.d_W.p, st, terms);
    launch_mixture(s, gp, lm ? k_lm_cost_mixture : k_chi2_mixture, st, terms);      // the component selected at st
    launch_robust(s, gp, lm ? k_lm_cost_robust : k_chi2_robust, st, terms);         // rho(r^T W0 r) in place of the weighted slot's term
    if (lm && gp.gc_n > 0)            // rho_mu(r^T W0 r): the surrogate is LM's alone -- a chi^2 inside a GNC run is the plain one (k_gnc_final put the plain W back)
        launch_gnc(s, gp, k_gnc_cost, (const int *)gp.d_fa.p, (const int *)gp.d_fb.p, (const double *)gp.d_z.p, st, terms);
    launch_polar(s, gp, k_chi2_polar, st, terms);                                   // r_p' Wp r_p in place of the slot's term
    launch_gaussian(s, gp, k_chi2_gaussian, st, terms);                             // c0 - 2 eta' delta + delta' Lambda delta on the factor's first entry
}

// The one reducer: n doubles at `in` -> *out by sum, max (n >= 1) or min, in one stage up to REDUCE_SPLIT terms and through REDUCE_PARTS
// partial results at `parts` above it (kernels.hip.h: reduce_one / reduce_parts)
enum ReduceOp { REDUCE_SUM, REDUCE_MAX, REDUCE_MIN };
static void enqueue_reduce(ReduceOp op, hipStream_t s, int n, const double *in, double *parts, double *out) {
    auto *const one = op == REDUCE_SUM ? k_reduce : op == REDUCE_MAX ? k_gnc_max : k_chordal_min;
    auto *const many = op == REDUCE_SUM ? k_reduce_parts : op == REDUCE_MAX ? k_gnc_max_parts : k_chordal_min_parts;
    if (n > REDUCE_SPLIT) {
        hipLaunchKernelGGL(many, dim3(REDUCE_PARTS), dim3(TPB), 0, s, n, in, parts);
        hipLaunchKernelGGL(one, dim3(1), dim3(1024), 0, s, REDUCE_PARTS, (const double *)parts, out);
    } else hipLaunchKernelGGL(one, dim3(1), dim3(1024), 0, s, n, in, out);
}

static double device_chi2(GraphPack &gp) {     // chi^2 at d_state; synchronises the stream
    hipStream_t s = gp.stream;
    if (gp.F == 0) return 0;
    enqueue_objective(gp, s, Convention::CHI2, gp.d_state.p, gp.d_chi2f.p);
    enqueue_reduce(REDUCE_SUM, s, gp.F, gp.d_chi2f.p, gp.d_chi2f.p + gp.F_cap, gp.d_scalar.p);      // (the parts live behind the F_cap per-factor terms: upload_factors)
    HIPCHECK(hipMemcpyAsync(gp.h_scalar.p, gp.d_scalar.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return gp.h_scalar.p[0];
}

// what fills the contribution slots of a Gauss-Newton step: the families' slots, the linearisation (+ the host-evaluated factors' blocks),
// the families' contributions and the fixed-node mask
static void enqueue_linearise(Context &c, GraphPack &gp, hipStream_t s, bool unary_at_lp) {
    const int F = c.plan.F;
    enqueue_families_before(gp, s, unary_at_lp ? gp.d_upt.p : (const double *)nullptr);
    // (a variant of the kernel without the asymmetric-W orientation branch, for graphs that have no such factor, was measured in round 6: no
    // difference -- 0.79 ms on the 1 M lattice either way)
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((F + TPB - 1) / TPB), dim3(TPB), 0, s, 0, F, (const int *)nullptr, gp.d_fa.p, gp.d_fb.p, gp.d_z.p, gp.d_W.p,
                           gp.d_lp.p, gp.d_state.p, c.d_swap.p, c.dp.slot_blk, c.dp.slot_rhs, c.d_H.p, c.d_bad.p, unary_at_lp ? gp.d_upt.p : (const double *)nullptr, c.d_epoch.p);
    };
    if (F >= g_opt.linearize_staged_min) launch(k_linearize_t<true>); else launch(k_linearize_t<false>);
    if (!gp.host_idx.empty()) {         // host-evaluated factors: their blocks replace the null contributions written above
        const int nh = (int)gp.host_idx.size();
        HIPCHECK(hipMemcpyAsync(gp.d_hostH.p, gp.h_hostH.p, (size_t)33 * 8 * nh, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_scatter_host, dim3((nh + TPB - 1) / TPB), dim3(TPB), 0, s, nh, gp.d_host_idx.p, gp.d_hostH.p, gp.d_fb.p, c.d_swap.p,
                           c.dp.slot_blk, c.dp.slot_rhs, c.d_H.p);
    }
    enqueue_families_after(c, gp, s);
}

// what a caller of the numeric phase asks for beyond the plain step; everything is off unless named
struct NumericArgs {
    hipEvent_t *ev = nullptr;                        // record stage events (0 start, 1 after linearise, 2 after factor, 3 after solve+update)
    bool unary_at_lp = false;                        // unary factors are linearised at gp.d_upt
    bool ktime = false;                              // bracket EVERY kernel launch with its own HIP event pair on this stream (c.k_ev / c.k_ids)
    bool io_host = false;                            // the API call's form: states in from the pinned mirror, new states / dx / pivot flag out to pinned mirrors
    bool relin = false;                              // the state update leaves the new states in the l_points as well (resident loop)
    double *st_dest = nullptr;                       // (LM iterations, solver_lm.inc.h) where the state update writes x (+) h instead of d_state -- the trial buffer
    const std::function<void()> *fill = nullptr;     // (chordal initialisation, solver_chordal.inc.h) what fills the contribution slots, clears the failure record and advances the step counter in place of enqueue_linearise
};
// enqueue: linearise -> per level {assemble+factor} -> back substitution -> state update
static void enqueue_numeric(Context &c, GraphPack &gp, hipStream_t s, const NumericArgs &a = NumericArgs{}) {
    const Plan &P = c.plan;
    const int N = P.N;
    const bool io_host = a.io_host;
    KTimer kt;
    if (a.ktime) { c.k_ids.clear(); c.k_lev.clear(); kt.c = &c; kt.s = s; }
    if (a.ev) HIPCHECK(hipEventRecord(a.ev[0], s));
    if (c.dp.prof) HIPCHECK(hipMemsetAsync(c.d_prof.p, 0, (size_t)8 * PROF_SLOTS * P.nF, s));
    if (io_host) hipLaunchKernelGGL(k_load_states, dim3((3 * N + TPB - 1) / TPB), dim3(TPB), 0, s, 3 * N, gp.h_state.p, gp.d_state.p, gp.d_lp.p);
    enqueue_poison(c, s, nullptr, P.nF);
    kt.tic(K_LINEARIZE);
    if (a.fill) (*a.fill)(); else enqueue_linearise(c, gp, s, a.unary_at_lp);
    kt.toc();
    if (a.ev) HIPCHECK(hipEventRecord(a.ev[1], s));
    const int l0 = c.persist_l0 >= 0 ? c.persist_l0 : P.nLevels;        // levels >= l0: one multi-level launch each way
    const int ul0 = l0 < P.nLevels ? c.persist_up_l0 : l0;              // ... the factorisation's may hold level 0 as well (option persist_up)
    for (int l = 0; l < ul0; l++) {
        kt.level = l;
        if (l == 0 && c.x_leaf_n > 0) { kt.tic(K_FRONT_SMALL); launch_front_small(c, c.levels[0], s, nullptr, c.x_leaf_off, c.x_leaf_n); kt.toc(); }      // (small fronts only)
        else enqueue_factor_level(c, c.levels[l], s, kt);
    }
    kt.level = ul0;
    if (l0 < P.nLevels) { kt.tic(K_FRONT_SMALL); launch_front_persist(c, s); kt.toc(); }
    if (a.ev) HIPCHECK(hipEventRecord(a.ev[2], s));
    // the state update of a front's own poses rides on its back substitution (no kernel of its own); the last launch also
    // mirrors the pivot flag for the API call
    UpdArgs upd{ c.d_perm.p, gp.d_lp.p, a.st_dest ? a.st_dest : gp.d_state.p, gp.d_dx.p, io_host ? gp.h_lp.p : nullptr, io_host ? gp.h_dx.p : nullptr, nullptr, a.relin ? gp.d_lp.p : nullptr };
    const int dl0 = l0 < P.nLevels ? c.persist_dn_l0 : l0;              // ... the back substitution's may hold level 0 as well (option persist_leaves)
    if (l0 < P.nLevels) {
        UpdArgs u = upd; if (dl0 == 0) u.bad_out = io_host ? c.h_bad.p : nullptr;
        kt.tic(K_BACKSOLVE);
        const bool xp = c.x_dn_n > 0;                            // the XCD-placed list (empty slots included)
        launch_backsolve_multi(c, s, persist_plan(c), c.d_tab.p + (xp ? c.x_dn_off : c.p_dn_off), xp ? c.x_dn_n : c.p_dn_n, c.p_dn_lds, c.p_dn_maxns, c.d_flags.p + c.flag_stride, u);
        kt.toc();
    }
    for (int l = dl0 - 1; l >= 0; l--) {
        UpdArgs u = upd; if (l == 0) u.bad_out = io_host ? c.h_bad.p : nullptr;
        kt.level = l;
        if (l == 0 && c.x_leaf_n > 0) launch_backsolve(c, c.levels[0], s, kt, nullptr, u, c.x_leaf_off, c.x_leaf_n);
        else launch_backsolve(c, c.levels[l], s, kt, nullptr, u);
    }
    if (a.ev) HIPCHECK(hipEventRecord(a.ev[3], s));
    HIPCHECK(hipGetLastError());
}
// after the stream was synchronised: fold the event pairs of the last instrumented enqueue into c.k_ms
static void collect_kernel_times(Context &c) {
    for (size_t i = 0; i < c.k_ids.size(); i++) {
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, c.k_ev[2 * i], c.k_ev[2 * i + 1]));
        c.k_ms[c.k_ids[i]] += ms; c.k_calls[c.k_ids[i]]++;
        const int l = i < c.k_lev.size() ? c.k_lev[i] : -1;
        if (l >= 0) {
            if (c.lev_up_ms.size() <= (size_t)l) { c.lev_up_ms.resize(l + 1, 0.0); c.lev_dn_ms.resize(l + 1, 0.0); }
            (c.k_ids[i] == K_BACKSOLVE ? c.lev_dn_ms : c.lev_up_ms)[l] += ms;
        }
    }
    c.k_ids.clear();
}

// Run what `enqueue` puts on stream s as the captured hipGraph g, which depends on `key`: a graph captured with another key is retired
// (Captured::fit, which also says when a run is not worth a graph: enqueued directly then); captured and instantiated when g holds none; launched.
template <class Enqueue> static void replay_captured(Context &c, Context::Captured &g, const CaptureKey &key, hipStream_t s, Enqueue enqueue) {
    if (!g.fit(c, key)) { enqueue(); return; }
    if (!g.exec) {
        hipGraph_t graph = nullptr;
        HIPCHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        enqueue();
        HIPCHECK(hipStreamEndCapture(s, &graph));
        HIPCHECK(hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0));
        HIPCHECK(hipGraphDestroy(graph));
        c.n_captures++;
    }
    c.graph_stream = s;
    HIPCHECK(hipGraphLaunch(g.exec, s));
}

long long graph_captures(const april_graph_cholesky_param_t *param) { return context_field(param, [](const Context &c) { return c.n_captures; }); }

// run the numeric phase, replaying a captured hipGraph when enabled.  timing: record the stage events c.ev; ktime: an event pair around every
// kernel (neither is ever captured); the rest as NumericArgs (io_host: the other two do not apply)
struct RunArgs { bool timing = false, ktime = false, unary_at_lp = false, io_host = false, relin = false; };
static void run_numeric(Context &c, GraphPack &gp, const RunArgs &r = RunArgs{}) {
    hipStream_t s = gp.stream;
    set_small_attr();
    rewind_epoch(c, s, 1);
    if (r.timing && !c.have_events) { for (auto &e : c.ev) HIPCHECK(hipEventCreate(&e)); c.have_events = true; }
    NumericArgs a;
    a.io_host = r.io_host;
    if (!r.io_host) a.relin = r.relin;
    const bool graph = g_opt.use_graph && !r.timing && !r.ktime && gp.host_idx.empty();      // (host-evaluated factors: staging buffers may move)
    Context::Captured *cap = !graph ? nullptr : r.io_host ? &c.cap_api : !r.unary_at_lp ? &c.cap_step : nullptr;
    if (cap) {
        const CaptureKey key = r.io_host ? gp.capture_key({ (size_t)gp.h_state.p, (size_t)gp.h_lp.p, (size_t)gp.h_dx.p, (size_t)c.h_bad.p, (size_t)gp.N }) : gp.capture_key();
        replay_captured(c, *cap, key, s, [&] { enqueue_numeric(c, gp, s, a); });      // (API calls: not the first one with a new key -- every fall-back of an incremental run, every cold call)
    } else {
        a.ev = r.timing ? c.ev : nullptr; a.ktime = r.ktime;
        if (!r.io_host) a.unary_at_lp = r.unary_at_lp;
        enqueue_numeric(c, gp, s, a);
    }
}
