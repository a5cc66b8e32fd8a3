// symbolic.cpp — supernodal symbolic analysis on the pose-block graph (host, C++).
//
// Counterpart of the reference's symbolic stages: cs_schol (csparse.c:1693: etree, postorder, column
// counts), search_tree_create_from_smat (aprilsam.c:613-657: block elimination tree) and the idxs
// numbering (aprilsam.c:141-148) — restructured for a multifrontal GPU factorisation: every nested-
// dissection tree node is ONE dense front; we compute each front's update-row structure, the assembly
// tree, child->parent scatter maps, the factor->front assignment with deterministic gather lists, and a
// level schedule (fronts of one level are independent => one batched kernel launch).
#include "plan.h"
#include "solver.h"
#include "errors.h"

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <chrono>
#include <mutex>

namespace asam {

// Separator amalgamation (option amalg).  On a graph the size of M3500 nothing is bound by flops: the factorisation is a chain of
// dependent fronts, and a front on that chain costs about HAND = 12 us of hand-over (flag, extend-add of the children's blocks from
// memory, store + release of its update block) plus PERCOL = 0.19 us per own column (the in-register pivot chains;
// profiles/r05_front_times_m3500.txt), the back substitution another 2.7 us + 0.8 us per 64 columns.  A separator front that takes in a
// child SEPARATOR -- one dense front whose own part is the child separators first, then its own: a valid supernode, the blocks between two
// child separators are structural zeros treated as dense -- removes one hand-over from the path for the price of the child's columns on the
// parent's chain.  Bottom-up over the dissection tree with that model: cost(n) = hand + percol * own(n) + max over children cost(c); a node
// tries to take in its 1, 2, ... most expensive separator children (they sit on its critical path; a taken child brings the separators it
// took in itself, and its remaining children become n's) and keeps the prefix with the lowest cost(n), as long as the merged front still
// fits the single-workgroup kernel in panel mode (own columns x all rows in LDS; rows = own + the region's boundary, counted here) and owns
// at most amalg_max poses.  Leaves are never merged: they hold most of the poses and run side by side.  M3500: 9 levels -> 5-6.
static void amalgamate(NDTree &tree, int N, const std::vector<int> &ap, const std::vector<int> &ai, int max_own, size_t lds_budget) {
    const double HAND = 12.0 + 2.7, PERCOL = 0.19 + 0.8 / 64.0;         // us, up-sweep + down-sweep
    constexpr int REGION_MAX = 4096;                                      // subtrees with more poses are not looked at (their separators are far too wide to merge)
    const int nT = (int)tree.nodes.size();
    // post-order
    std::vector<int> order; order.reserve(nT);
    {
        std::vector<std::pair<int, size_t>> st;
        for (int r : tree.roots) {
            st.push_back({ r, 0 });
            while (!st.empty()) {
                auto &top = st.back();
                const NDTree::Node &nd = tree.nodes[top.first];
                if (top.second < nd.children.size()) { const int c = nd.children[top.second++]; st.push_back({ c, 0 }); continue; }
                order.push_back(top.first); st.pop_back();
            }
        }
    }
    std::vector<int> region(nT, 0);                                       // poses in the subtree
    for (int n : order) { region[n] = (int)tree.nodes[n].verts.size(); for (int c : tree.nodes[n].children) region[n] += region[c]; }
    // boundary of a subtree's region = update rows of its top front (the region is eliminated completely below it)
    std::vector<int> stamp_in(N, -1), stamp_b(N, -1), bnd(nT, -1);
    std::vector<int> stk, verts;
    auto boundary = [&](int n) {
        verts.clear(); stk.assign(1, n);
        while (!stk.empty()) { const int k = stk.back(); stk.pop_back(); for (int v : tree.nodes[k].verts) { stamp_in[v] = n; verts.push_back(v); } for (int c : tree.nodes[k].children) stk.push_back(c); }
        int cnt = 0;
        for (int v : verts) for (int e = ap[v]; e < ap[v + 1]; e++) { const int u = ai[e]; if (stamp_in[u] != n && stamp_b[u] != n) { stamp_b[u] = n; cnt++; } }
        return cnt;
    };
    std::vector<double> cost(nT, 0.0);
    std::vector<char> dead(nT, 0);
    for (int n : order) {
        NDTree::Node &nd = tree.nodes[n];
        auto eval = [&](size_t own, const std::vector<int> &kids) { double m = 0; for (int c : kids) m = std::max(m, cost[c]); return HAND + PERCOL * 3.0 * (double)own + m; };
        cost[n] = eval(nd.verts.size(), nd.children);
        if (nd.children.empty() || region[n] > REGION_MAX) continue;
        std::vector<int> seps;
        for (int c : nd.children) if (!tree.nodes[c].children.empty()) seps.push_back(c);
        if (seps.empty()) continue;
        std::sort(seps.begin(), seps.end(), [&](int a, int b) { return cost[a] != cost[b] ? cost[a] > cost[b] : a < b; });
        if (bnd[n] < 0) bnd[n] = boundary(n);
        size_t own = nd.verts.size();
        std::vector<int> kids = nd.children;
        double best = cost[n]; size_t best_k = 0;
        for (size_t k = 0; k < seps.size(); k++) {
            const NDTree::Node &ch = tree.nodes[seps[k]];
            own += ch.verts.size();
            const size_t R = 3 * (own + (size_t)bnd[n] + 1);
            if (own > (size_t)max_own || (R | 1) * 3 * own * 8 > lds_budget) break;
            kids.erase(std::find(kids.begin(), kids.end(), seps[k]));
            kids.insert(kids.end(), ch.children.begin(), ch.children.end());
            const double cst = eval(own, kids);
            if (cst < best - 1e-9) { best = cst; best_k = k + 1; }
        }
        if (!best_k) continue;
        std::vector<int> vs;
        for (size_t k = 0; k < best_k; k++) {
            NDTree::Node &ch = tree.nodes[seps[k]];
            vs.insert(vs.end(), ch.verts.begin(), ch.verts.end());
            nd.children.erase(std::find(nd.children.begin(), nd.children.end(), seps[k]));
            nd.children.insert(nd.children.end(), ch.children.begin(), ch.children.end());
            dead[seps[k]] = 1; ch.verts.clear(); ch.children.clear();
        }
        vs.insert(vs.end(), nd.verts.begin(), nd.verts.end());
        nd.verts.swap(vs);
        cost[n] = best;
    }
    std::vector<int> remap(nT, -1);
    int w = 0;
    for (int i = 0; i < nT; i++) if (!dead[i]) { remap[i] = w; if (w != i) tree.nodes[w] = std::move(tree.nodes[i]); w++; }
    tree.nodes.resize(w);
    for (auto &nd : tree.nodes) for (int &c : nd.children) c = remap[c];
    for (int &r : tree.roots) r = remap[r];
}

void build_plan(Plan &P, int N, int F, const int *fn, const double *xy, int leaf_nodes) {
    // one plan at a time: the dissection and the symbolic phases share ONE pool of planner threads (ordering.cpp: PlanPool) -- calls
    // from threads that drive different devices queue up here, everything else they do runs side by side
    static std::mutex build_mu;
    std::lock_guard<std::mutex> build_lock(build_mu);
    P = Plan();
    P.N = N; P.F = F; P.leaf_nodes = leaf_nodes;
    if (N <= 0) return;
    // APRILSAM_AMD_PLAN_PROFILE: wall-clock split of the planner phases on stderr
    const bool prof = getenv("APRILSAM_AMD_PLAN_PROFILE") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tph[8]; int nph = 0;
    auto stamp = [&] { if (prof && nph < 8) tph[nph++] = now(); };
    stamp();

    PlanSession session(N);              // the planner's worker threads stay awake for the length of this plan (ordering.cpp)
    // ---- pose adjacency (deduplicated CSR) ------------------------------------------------------------
    std::vector<int> ap(N + 1, 0), ai;
    {
        std::vector<int> deg(N, 0);
        for (int f = 0; f < F; f++) { int a = fn[2 * f], b = fn[2 * f + 1]; if (b >= 0 && a != b) { deg[a]++; deg[b]++; } }
        for (int i = 0; i < N; i++) ap[i + 1] = ap[i] + deg[i];
        ai.resize(ap[N]);
        std::vector<int> fill(ap.begin(), ap.end() - 1);
        for (int f = 0; f < F; f++) { int a = fn[2 * f], b = fn[2 * f + 1]; if (b >= 0 && a != b) { ai[fill[a]++] = b; ai[fill[b]++] = a; } }
        // sort + unique per row, then compact
        std::vector<int> np(N + 1, 0); int w = 0;
        for (int i = 0; i < N; i++) {
            std::sort(ai.begin() + ap[i], ai.begin() + ap[i + 1]);
            int last = -1;
            for (int e = ap[i]; e < ap[i + 1]; e++) if (ai[e] != last) { last = ai[e]; ai[w++] = last; }
            np[i + 1] = w;
        }
        ai.resize(w); ap.swap(np);
    }

    stamp();
    // ---- nested dissection tree, post-order numbering ----------------------------------------------
    NDTree tree;
    // Option pin_last = k ("recent poses last", the counterpart of the reference's constrained min-degree order,
    // aprilsam.c:1021-1098, which keeps the newest pose and the poses around its neighbours at the end of the elimination
    // order): the k highest pose ids are taken out of the dissection and form the ROOT front, so that a factor arriving at
    // the newest poses only touches the root.  Measured on the incremental demo: tools/inc_hist.py -> profiles/.
    const int pin = std::max(0, std::min(g_opt.pin_last, N - 1));
    if (pin > 0) {
        const int M = N - pin;
        std::vector<int> ap2(M + 1, 0), ai2;
        for (int i = 0; i < M; i++) { for (int e = ap[i]; e < ap[i + 1]; e++) if (ai[e] < M) ai2.push_back(ai[e]); ap2[i + 1] = (int)ai2.size(); }
        nested_dissection(M, ap2, ai2, xy, leaf_nodes, tree);
        NDTree::Node root;
        for (int v = M; v < N; v++) root.verts.push_back(v);
        root.children = tree.roots;
        tree.nodes.push_back(std::move(root));
        tree.roots.assign(1, (int)tree.nodes.size() - 1);
    } else
        nested_dissection(N, ap, ai, xy, leaf_nodes, tree);
    if (g_opt.amalg > 0) {          // (the LDS of a 16-wave workgroup's work lists comes off the budget: kernels.hip.h wl_bytes)
        const size_t wl = 64 * 24 + 16 * (128 * 8 + 64 * 8);
        amalgamate(tree, N, ap, ai, std::max(g_opt.amalg_max, 1), (size_t)std::max(g_opt.small_lds_kb, 32) * 1024 - wl);
    }
    const int nT = (int)tree.nodes.size();
    P.nF = nT;
    P.perm.assign(N, -1); P.pos.assign(N, -1);
    P.f_first.assign(nT, 0); P.f_nsb.assign(nT, 0);
    std::vector<int> tfront(nT, -1);        // ND tree node -> front index (post-order)
    {
        int nextpos = 0, nextfront = 0;
        std::vector<std::pair<int, size_t>> st;     // (tree node, next child)
        for (int r : tree.roots) {
            st.push_back({ r, 0 });
            while (!st.empty()) {
                auto &top = st.back();
                NDTree::Node &nd = tree.nodes[top.first];
                if (top.second < nd.children.size()) { int c = nd.children[top.second++]; st.push_back({ c, 0 }); continue; }
                int t = nextfront++;
                tfront[top.first] = t;
                P.f_first[t] = nextpos; P.f_nsb[t] = (int)nd.verts.size();
                for (int v : nd.verts) { P.perm[nextpos] = v; P.pos[v] = nextpos; nextpos++; }
                st.pop_back();
            }
        }
        assert(nextpos == N && nextfront == nT);
    }
    std::vector<int> pos_front(N);
    for (int t = 0; t < nT; t++) for (int k = 0; k < P.f_nsb[t]; k++) pos_front[P.f_first[t] + k] = t;

    stamp();
    // ---- structure of every front (block positions > own range), assembly tree -----------------------
    P.f_nub.assign(nT, 0); P.f_parent.assign(nT, -1); P.f_rows_ptr.assign(nT + 1, 0);
    std::vector<std::vector<int>> kids(nT);
    std::vector<int> mark(N, -1), tmp;
    std::vector<std::vector<int>> strct(nT);
    for (int t = 0; t < nT; t++) {
        const int last = P.f_first[t] + P.f_nsb[t] - 1;
        tmp.clear();
        for (int p = P.f_first[t]; p <= last; p++) {
            int v = P.perm[p];
            for (int e = ap[v]; e < ap[v + 1]; e++) { int q = P.pos[ai[e]]; if (q > last && mark[q] != t) { mark[q] = t; tmp.push_back(q); } }
        }
        for (int c : kids[t]) for (int q : strct[c]) if (q > last && mark[q] != t) { mark[q] = t; tmp.push_back(q); }
        std::sort(tmp.begin(), tmp.end());
        strct[t] = tmp;
        P.f_nub[t] = (int)tmp.size();
        if (!tmp.empty()) { int par = pos_front[tmp[0]]; assert(par > t); P.f_parent[t] = par; kids[par].push_back(t); }
    }
    for (int t = 0; t < nT; t++) P.f_rows_ptr[t + 1] = P.f_rows_ptr[t] + P.f_nub[t];
    P.f_rows.resize(P.f_rows_ptr[nT]); P.f_rel.assign(P.f_rows_ptr[nT], -1);
    for (int t = 0; t < nT; t++) std::copy(strct[t].begin(), strct[t].end(), P.f_rows.begin() + P.f_rows_ptr[t]);

    auto local_index = [&](int t, int p) -> int {      // block index of position p inside front t (or -1)
        if (p >= P.f_first[t] && p < P.f_first[t] + P.f_nsb[t]) return p - P.f_first[t];
        const int *b = P.f_rows.data() + P.f_rows_ptr[t], *e = b + P.f_nub[t];
        const int *it = std::lower_bound(b, e, p);
        if (it == e || *it != p) return -1;
        return P.f_nsb[t] + (int)(it - b);
    };
    for (int t = 0; t < nT; t++) {
        int par = P.f_parent[t];
        for (int64_t k = P.f_rows_ptr[t]; k < P.f_rows_ptr[t + 1]; k++) {
            int li = local_index(par, P.f_rows[k]);
            if (li < 0) fail(ERR_INTERNAL, "symbolic inconsistency (front %d row %d)", t, P.f_rows[k]);
            P.f_rel[k] = li;
        }
    }
    P.ch_ptr.assign(nT + 1, 0);
    for (int t = 0; t < nT; t++) P.ch_ptr[t + 1] = P.ch_ptr[t] + (int)kids[t].size();
    P.ch_idx.resize(P.ch_ptr[nT]);
    for (int t = 0; t < nT; t++) std::copy(kids[t].begin(), kids[t].end(), P.ch_idx.begin() + P.ch_ptr[t]);

    stamp();
    // ---- levels ------------------------------------------------------------------------------------------
    P.f_level.assign(nT, 0);
    for (int t = 0; t < nT; t++) { int par = P.f_parent[t]; if (par >= 0) P.f_level[par] = std::max(P.f_level[par], P.f_level[t] + 1); }
    P.nLevels = 0;
    for (int t = 0; t < nT; t++) P.nLevels = std::max(P.nLevels, P.f_level[t] + 1);
    P.lev_ptr.assign(P.nLevels + 1, 0);
    for (int t = 0; t < nT; t++) P.lev_ptr[P.f_level[t] + 1]++;
    for (int l = 0; l < P.nLevels; l++) P.lev_ptr[l + 1] += P.lev_ptr[l];
    P.lev_fronts.resize(nT);
    { std::vector<int> fill(P.lev_ptr.begin(), P.lev_ptr.end() - 1); for (int t = 0; t < nT; t++) P.lev_fronts[fill[P.f_level[t]]++] = t; }

    stamp();
    // ---- factor -> front assignment + deterministic gather lists -------------------------------------
    P.fac_front.assign(F, -1); P.fac_la.assign(F, -1); P.fac_lb.assign(F, -1); P.fac_swap.assign(F, 0);
    std::atomic<int> lost{ -1 };
    plan_parallel_for(F, 4096, [&](int f0, int f1) {               // the searches, side by side ...
        for (int f = f0; f < f1; f++) {
            int a = fn[2 * f], b = fn[2 * f + 1];
            if (a < 0 || a >= N || b >= N || a == b) continue;          // malformed: ignored
            int pa = P.pos[a], pb = b >= 0 ? P.pos[b] : -1;
            int t = pos_front[(pb >= 0 && pb < pa) ? pb : pa];
            int la = local_index(t, pa), lb = pb >= 0 ? local_index(t, pb) : -1;
            if (la < 0 || (pb >= 0 && lb < 0)) { lost.store(f); continue; }
            P.fac_front[f] = t; P.fac_la[f] = la; P.fac_lb[f] = lb;
        }
    });
    if (lost.load() >= 0) fail(ERR_INTERNAL, "factor %d not inside its front", lost.load());
    for (int f = 0; f < F; f++) if (P.fac_front[f] >= 0 && P.fac_lb[f] >= 0) P.fac_swap[f] = P.fac_la[f] < P.fac_lb[f];
    // packed sort keys below: 16 bits of local block column, 17 of local block row + 1, 30 of contribution id, 1 of kind.  (Round 6: the id had
    // 26 bits -- 22 million factors -- which a 2 500 x 2 500 lattice exceeds while its 190 GB of fronts still fit one MI355X.)
    constexpr int KEY_SRC_BITS = 30, KEY_ROW_BITS = 17, KEY_COL_BITS = 16;
    static_assert(1 + KEY_SRC_BITS + KEY_ROW_BITS + KEY_COL_BITS == 64 && sizeof(unsigned long long) == 8, "packed sort keys");
    if ((size_t)3 * F >= (1u << KEY_SRC_BITS) || (size_t)5 * F >= 0x7fffffffu)
        fail(ERR_UNSUPPORTED, "%d factors: this build handles up to %u (packed sort keys of the symbolic analysis)", F, (1u << KEY_SRC_BITS) / 3 - 1);
    for (int t = 0; t < nT; t++)
        if (P.f_nsb[t] + P.f_nub[t] + 1 >= (1 << KEY_COL_BITS))
            fail(ERR_UNSUPPORTED, "front %d has %d block rows: this build handles up to %d (packed sort keys of the symbolic analysis)", t, P.f_nsb[t] + P.f_nub[t] + 1, (1 << KEY_COL_BITS) - 1);
    P.bd_front_ptr.clear(); P.rd_front_ptr.clear();       // (the per-kind gather lists are derived on demand: build_gather_lists)

    stamp();
    // ---- unified destination records + contribution slots (device layout) --------------------------------
    {
        // One record per destination block (brow -1 = the rhs row) with the consecutive slots of its contributions.  Order inside a
        // front: (col, row with the rhs row first, contribution id) -- a counting sort by front, then a sort of 64-bit packed keys
        // inside every (small) bucket, the buckets side by side: several times faster than one comparison sort over all 5 F
        // entries, and planning sits on the cold-call path.
        std::vector<int> ptr(nT + 1, 0);
        for (int f = 0; f < F; f++) if (P.fac_front[f] >= 0) ptr[P.fac_front[f] + 1] += P.fac_lb[f] >= 0 ? 5 : 2;
        for (int t = 0; t < nT; t++) ptr[t + 1] += ptr[t];
        const size_t total = (size_t)ptr[nT];
        std::vector<unsigned long long> key(total);
        auto pack = [](int col, int row, int src, int rhs) {
            return ((unsigned long long)(unsigned)col << (1 + KEY_SRC_BITS + KEY_ROW_BITS)) | ((unsigned long long)(unsigned)(row + 1) << (1 + KEY_SRC_BITS)) | ((unsigned long long)(unsigned)src << 1) | (unsigned)rhs;
        };
        {
            std::vector<int> fill(ptr.begin(), ptr.end() - 1);
            for (int f = 0; f < F; f++) {
                const int t = P.fac_front[f], la = P.fac_la[f], lb = P.fac_lb[f];
                if (t < 0) continue;
                int &w = fill[t];
                key[w++] = pack(la, la, 3 * f + 0, 0); key[w++] = pack(la, -1, 2 * f + 0, 1);
                if (lb >= 0) {
                    key[w++] = pack(std::min(la, lb), std::max(la, lb), 3 * f + 1, 0);
                    key[w++] = pack(lb, lb, 3 * f + 2, 0); key[w++] = pack(lb, -1, 2 * f + 1, 1);
                }
            }
        }
        auto same_dest = [](unsigned long long a, unsigned long long b) { return (a >> (1 + KEY_SRC_BITS)) == (b >> (1 + KEY_SRC_BITS)); };     // same (col, row)
        P.dest_front_ptr.assign(nT + 1, 0);
        plan_parallel_for(nT, 64, [&](int t0, int t1) {
            for (int t = t0; t < t1; t++) {
                std::sort(key.begin() + ptr[t], key.begin() + ptr[t + 1]);
                int fresh = 0;
                for (int i = ptr[t]; i < ptr[t + 1]; i++) fresh += i == ptr[t] || !same_dest(key[i], key[i - 1]);
                P.dest_front_ptr[t + 1] = fresh;
            }
        });
        for (int t = 0; t < nT; t++) P.dest_front_ptr[t + 1] += P.dest_front_ptr[t];
        P.dest.resize((size_t)P.dest_front_ptr[nT]);
        P.slot_blk.assign((size_t)3 * F, -1); P.slot_rhs.assign((size_t)2 * F, -1);
        plan_parallel_for(nT, 64, [&](int t0, int t1) {
            for (int t = t0; t < t1; t++) {
                int d = P.dest_front_ptr[t] - 1;
                for (int i = ptr[t]; i < ptr[t + 1]; i++) {
                    const unsigned long long k = key[i];
                    const int col = (int)(k >> (1 + KEY_SRC_BITS + KEY_ROW_BITS)), row = (int)((k >> (1 + KEY_SRC_BITS)) & ((1u << KEY_ROW_BITS) - 1)) - 1,
                              src = (int)((k >> 1) & ((1u << KEY_SRC_BITS) - 1)), rhs = (int)(k & 1);
                    if (i == ptr[t] || !same_dest(k, key[i - 1])) P.dest[++d] = { row, col, i, i };
                    P.dest[d].src_end = i + 1;
                    (rhs ? P.slot_rhs : P.slot_blk)[src] = i;
                }
            }
        });
        P.n_slots = (int)total;
    }

    stamp();
    // ---- HBM pool offsets + statistics -----------------------------------------------------------------
    P.f_off.assign(nT, 0);
    int64_t off = 0;
    P.max_rows = 0; P.nnzL = 0; P.flops = 0;
    for (int t = 0; t < nT; t++) {
        P.f_off[t] = off;
        int64_t sz = (int64_t)P.rows(t) * P.cols(t);
        off += (sz + 31) & ~int64_t(31);                          // 256-byte aligned fronts
        int ns = 3 * P.f_nsb[t], nu = 3 * P.f_nub[t];
        P.max_rows = std::max(P.max_rows, ns + nu);
        P.nnzL += (int64_t)ns * (ns + 1) / 2 + (int64_t)nu * ns;
        for (int q = 0; q < ns; q++) { double c = (double)(ns - q) + nu; P.flops += c * c; }
    }
    P.pool_doubles = off;
    stamp();
    if (prof && nph == 8)
        fprintf(stderr, "aprilsam_amd planner N=%d F=%d: adjacency %.3f dissection %.3f front structure %.3f levels %.3f factor lists %.3f records+slots %.3f offsets %.3f | total %.3f ms\n",
                N, F, tph[1] - tph[0], tph[2] - tph[1], tph[3] - tph[2], tph[4] - tph[3], tph[5] - tph[4], tph[6] - tph[5], tph[7] - tph[6], tph[7] - tph[0]);
}

// The per-kind gather lists (block destinations / rhs destinations with their contributing factors in a fixed order): a
// restatement of the destination records for the host-side emulator of the tests (aprilsam_amd_plan_query "bd_*" / "rd_*");
// the device never reads them, so they are derived on demand.
void build_gather_lists(Plan &P) {
    if (!P.bd_front_ptr.empty()) return;
    const int F = P.F, nT = P.nF;
    struct Dest { int front, col, row, src; };
    std::vector<Dest> bd, rd; bd.reserve((size_t)3 * F); rd.reserve((size_t)2 * F);
    for (int f = 0; f < F; f++) {
        const int t = P.fac_front[f], la = P.fac_la[f], lb = P.fac_lb[f];
        if (t < 0) continue;
        bd.push_back({ t, la, la, 3 * f + 0 });
        rd.push_back({ t, la, 0, 2 * f + 0 });
        if (lb >= 0) {
            bd.push_back({ t, std::min(la, lb), std::max(la, lb), 3 * f + 1 });
            bd.push_back({ t, lb, lb, 3 * f + 2 });
            rd.push_back({ t, lb, 0, 2 * f + 1 });
        }
    }
    auto sort_dests = [&](std::vector<Dest> &v) {
        std::vector<int> ptr(nT + 1, 0);
        for (const Dest &d : v) ptr[d.front + 1]++;
        for (int t = 0; t < nT; t++) ptr[t + 1] += ptr[t];
        std::vector<unsigned long long> key(v.size());
        { std::vector<int> fill(ptr.begin(), ptr.end() - 1);
          for (const Dest &d : v) key[fill[d.front]++] = ((unsigned long long)(unsigned)d.col << 44) | ((unsigned long long)(unsigned)(d.row + 1) << 26) | (unsigned)d.src; }
        for (int t = 0; t < nT; t++) {
            std::sort(key.begin() + ptr[t], key.begin() + ptr[t + 1]);
            for (int i = ptr[t]; i < ptr[t + 1]; i++) v[i] = { t, (int)(key[i] >> 44), (int)((key[i] >> 26) & 0x3ffff) - 1, (int)(key[i] & 0x3ffffff) };
        }
    };
    sort_dests(bd);
    sort_dests(rd);
    auto compress = [&](const std::vector<Dest> &v, std::vector<int> &front_ptr, std::vector<int> &row, std::vector<int> &col,
                        std::vector<int> &src_ptr, std::vector<int> &src) {
        front_ptr.assign(nT + 1, 0); row.clear(); col.clear(); src_ptr.clear(); src.clear();
        src_ptr.push_back(0);
        for (size_t i = 0; i < v.size(); i++) {
            bool fresh = i == 0 || v[i].front != v[i - 1].front || v[i].col != v[i - 1].col || v[i].row != v[i - 1].row;
            if (fresh) { if (i) src_ptr.push_back((int)src.size()); row.push_back(v[i].row); col.push_back(v[i].col); front_ptr[v[i].front + 1]++; }
            src.push_back(v[i].src);
        }
        if (!v.empty()) src_ptr.push_back((int)src.size());
        for (int t = 0; t < nT; t++) front_ptr[t + 1] += front_ptr[t];
    };
    std::vector<int> dummy_row;
    compress(bd, P.bd_front_ptr, P.bd_row, P.bd_col, P.bd_src_ptr, P.bd_src);
    compress(rd, P.rd_front_ptr, dummy_row, P.rd_col, P.rd_src_ptr, P.rd_src);
}

}  // namespace asam

namespace asam {

// ---- XCD placement (plan.h) ------------------------------------------------------------------------------------------------------------
XcdLists xcd_place(const std::vector<int> &up, const std::vector<int> &leaves, const int *parent, const int *nsb, int nF, int cap, int cap_leaf) {
    constexpr int NX = 8;                                    // XCDs: workgroups b and b + 8 share one
    const double HAND = 12.0, PERCOL = 0.19;                 // us per front of the up-sweep's path: amalgamate's model above (front stamps)
    auto cost = [&](int t) { return HAND + PERCOL * 3.0 * (double)nsb[t]; };
    XcdLists x;
    const int n = (int)up.size();
    std::vector<int> at((size_t)nF, -1);                     // front -> position in up
    for (int i = 0; i < n; i++) at[up[i]] = i;
    auto up_parent = [&](int i) { const int p = parent[up[i]]; return p >= 0 ? at[p] : -1; };
    // critical path of each subtree (children come first in up) and the child on it
    std::vector<double> cp(n, 0.0), best(n, 0.0);
    std::vector<int> heavy(n, -1);
    for (int i = 0; i < n; i++) {
        cp[i] = cost(up[i]) + best[i];
        const int p = up_parent(i);
        if (p >= 0 && (heavy[p] < 0 || cp[i] > best[p])) { best[p] = cp[i]; heavy[p] = i; }
    }
    // heavy paths, costliest first (the root's: the critical path); each starts in the emptiest class and spills when a class is full
    std::vector<int> heads;
    for (int i = 0; i < n; i++) { const int p = up_parent(i); if (p < 0 || heavy[p] != i) heads.push_back(i); }
    std::stable_sort(heads.begin(), heads.end(), [&](int a, int b) { return cp[a] > cp[b]; });
    std::vector<int> cls(n, 0), cnt(NX, 0);
    std::vector<double> load(NX, 0.0);
    const bool capped = n <= NX * cap;                       // (otherwise no placement holds the launch: balance only)
    auto room = [&](int c) { return !capped || cnt[c] < cap; };
    auto emptiest = [&](const std::vector<int> &cn, const std::vector<double> &ld) {
        int c = 0;
        for (int k = 1; k < NX; k++) if (cn[k] < cn[c] || (cn[k] == cn[c] && ld[k] < ld[c])) c = k;
        return c;
    };
    for (int h : heads) {
        int c = emptiest(cnt, load);
        for (int i = h; i >= 0; i = heavy[i]) {
            while (!room(c)) c = (c + 1) % NX;
            cls[i] = c; cnt[c]++; load[c] += cost(up[i]);
        }
    }
    // slots: a front of class c takes the first id 8 k + c above its class's last one and above every dependency's
    auto place = [&](bool down, std::vector<int> &list) {
        std::vector<int> id(n, -1), dep(n, -1), cur(NX, 0);
        int kmax = 0;
        for (int j = 0; j < n; j++) {
            const int i = down ? n - 1 - j : j, c = cls[i], p = up_parent(i);
            const int need = (down ? (p >= 0 ? id[p] : -1) : dep[i]) + 1;
            const int k = std::max(cur[c], need > c ? (need - c + NX - 1) / NX : 0);
            id[i] = NX * k + c; cur[c] = k + 1; kmax = std::max(kmax, k + 1);
            if (!down && p >= 0) dep[p] = std::max(dep[p], id[i]);
        }
        list.assign((size_t)NX * kmax, -1);
        for (int i = 0; i < n; i++) list[id[i]] = up[i];
    };
    place(false, x.up);
    place(true, x.dn);
    // leaves: their parent's class (the parent's extend-add then reads them from its own L2 across the launch boundary), costliest first
    std::vector<int> lv(leaves);
    std::stable_sort(lv.begin(), lv.end(), [&](int a, int b) { return cost(a) > cost(b); });
    std::vector<int> lcnt(NX, 0), lslot(lv.size());
    std::vector<double> lload(NX, 0.0);
    const bool lcapped = (long long)lv.size() <= (long long)NX * cap_leaf;
    int kmax = 0;
    for (size_t j = 0; j < lv.size(); j++) {
        const int p = parent[lv[j]] >= 0 ? at[parent[lv[j]]] : -1;
        int c = p >= 0 ? cls[p] : emptiest(lcnt, lload);
        while (lcapped && lcnt[c] >= cap_leaf) c = (c + 1) % NX;
        lslot[j] = NX * lcnt[c] + c; lcnt[c]++; lload[c] += cost(lv[j]); kmax = std::max(kmax, lcnt[c]);
    }
    x.leaf.assign((size_t)NX * kmax, -1);
    for (size_t j = 0; j < lv.size(); j++) x.leaf[lslot[j]] = lv[j];
    return x;
}

int xcd_check(const XcdLists &x, const std::vector<int> &up, const std::vector<int> &leaves, const int *parent, int nF, int cap, int cap_leaf) {
    constexpr int NX = 8;
    auto same_set = [&](const std::vector<int> &list, const std::vector<int> &old) {
        if (list.size() % NX) return false;
        std::vector<int> a, b(old);
        for (int t : list) { if (t >= 0) a.push_back(t); else if (t != -1) return false; }
        std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
        return a == b;
    };
    if (!same_set(x.up, up)) return -1;
    if (!same_set(x.dn, up)) return -2;
    if (!same_set(x.leaf, leaves)) return -3;
    std::vector<int> iu((size_t)nF, -1), id((size_t)nF, -1);
    for (size_t b = 0; b < x.up.size(); b++) if (x.up[b] >= 0) iu[x.up[b]] = (int)b;
    for (size_t b = 0; b < x.dn.size(); b++) if (x.dn[b] >= 0) id[x.dn[b]] = (int)b;
    for (int t : up) {
        const int p = parent[t];
        if (p >= 0 && iu[p] >= 0 && iu[t] >= iu[p]) return -4;          // up: every child below its parent
        if (p >= 0 && id[p] >= 0 && id[t] <= id[p]) return -5;          // down: every parent below its children
        if (iu[t] % NX != id[t] % NX) return -6;                        // one class per front in both sweeps
    }
    auto fits = [&](const std::vector<int> &list, size_t n, int c) {
        if (n > (size_t)NX * c) return true;
        std::vector<int> cnt(NX, 0);
        for (size_t b = 0; b < list.size(); b++) if (list[b] >= 0 && ++cnt[b % NX] > c) return false;
        return true;
    };
    if (!fits(x.up, up.size(), cap) || !fits(x.dn, up.size(), cap)) return -7;
    if (!fits(x.leaf, leaves.size(), cap_leaf)) return -8;
    return 0;
}

// ---- the back substitution's list with the leaves inside (plan.h) ------------------------------------------------------------------------
std::vector<int> dn_with_leaves(const std::vector<int> &dn, const std::vector<int> &leaf) {
    std::vector<int> list(dn);
    list.insert(list.end(), leaf.begin(), leaf.end());
    return list;
}

int dn_with_leaves_check(const std::vector<int> &list, const std::vector<int> &dn, const std::vector<int> &leaf, const int *parent, int nF, bool placed) {
    constexpr int NX = 8;
    if (list.size() != dn.size() + leaf.size() || (placed && (dn.size() % NX || leaf.size() % NX))) return -1;
    if (!std::equal(dn.begin(), dn.end(), list.begin())) return -2;              // the upper fronts keep their slots
    std::vector<int> id((size_t)nF, -1), want((size_t)nF, -1);
    for (size_t b = 0; b < list.size(); b++) {
        const int t = list[b];
        if (t == -1) continue;
        if (t < 0 || t >= nF || id[t] >= 0) return -3;                           // every front at most once
        id[t] = (int)b;
    }
    for (size_t b = 0; b < dn.size(); b++) if (dn[b] >= 0) want[dn[b]] = (int)(b % NX);
    for (size_t b = 0; b < leaf.size(); b++) if (leaf[b] >= 0) { if (leaf[b] >= nF || want[leaf[b]] >= 0) return -3; want[leaf[b]] = (int)(b % NX); }
    for (int t = 0; t < nF; t++) {
        if ((id[t] >= 0) != (want[t] >= 0)) return -4;                           // ... and exactly the fronts of the two lists
        if (id[t] < 0) continue;
        if (placed && id[t] % NX != want[t]) return -5;// one class per front, the one it has in its own list
        const int p = parent[t];
        if (p >= 0 && id[p] >= 0 && id[p] >= id[t]) return -6;                   // every parent below its children
        if (p >= 0 && id[p] < 0 && id[t] >= (int)dn.size()) return -7;           // a leaf's parent is in the launch
    }
    return 0;
}

// ---- the order of the up-sweep's one launch (plan.h: up_schedule) ----------------------------------------------------------------------------
namespace {
constexpr int UP_NX = 8;
// us: a front with children from its last child's end to its own (amalgamate's model, as in xcd_place), a front without children from start to
// end, and what a front with children does before it needs them (zero fill, factor blocks, work lists): profiles/persist_leaves.txt section 5
constexpr double UP_HAND = 12.0, UP_PERCOL = 0.19, UP_LEAF = 4.8, UP_LEAD = 4.3;

struct UpTree {
    int n = 0;
    std::vector<int> front, cls, par, first_kid, next_kid;      // per entry of `base` (its order kept): front, class, parent's entry or -1, child chain
    std::vector<double> cost, prio;
    UpTree(const std::vector<int> &base, const int *parent, const int *nsb, int nF) {
        std::vector<int> at((size_t)nF, -1);
        for (size_t b = 0; b < base.size(); b++) if (base[b] >= 0 && base[b] < nF) { at[base[b]] = (int)front.size(); front.push_back(base[b]); cls.push_back((int)(b % UP_NX)); }
        n = (int)front.size();
        par.assign(n, -1); first_kid.assign(n, -1); next_kid.assign(n, -1); cost.assign(n, UP_LEAF); prio.assign(n, 0.0);
        for (int i = n - 1; i >= 0; i--) {
            const int p = parent[front[i]] >= 0 ? at[parent[front[i]]] : -1;
            par[i] = p;
            if (p >= 0) { next_kid[i] = first_kid[p]; first_kid[p] = i; }
        }
        for (int i = 0; i < n; i++) if (first_kid[i] >= 0) cost[i] = UP_HAND + UP_PERCOL * 3.0 * (double)nsb[front[i]];
        // remaining path to the root's end, own cost included: parents first (they follow their children in base)
        for (int i = n - 1; i >= 0; i--) prio[i] = cost[i] + (par[i] >= 0 ? prio[par[i]] : 0.0);
    }
};
// place()'s rule of xcd_place in the order `seq`: the next id 8 k + c of the front's class above the class's last one and above every child's
std::vector<int> up_slots(const UpTree &T, const std::vector<int> &seq) {
    std::vector<int> id(T.n, -1), dep(T.n, -1), cur(UP_NX, 0);
    int kmax = 0;
    for (int i : seq) {
        const int c = T.cls[i], need = dep[i] + 1;
        const int k = std::max(cur[c], need > c ? (need - c + UP_NX - 1) / UP_NX : 0);
        id[i] = UP_NX * k + c; cur[c] = k + 1; kmax = std::max(kmax, k + 1);
        if (T.par[i] >= 0) dep[T.par[i]] = std::max(dep[T.par[i]], id[i]);
    }
    std::vector<int> list((size_t)UP_NX * kmax, -1);
    for (int i : seq) list[id[i]] = T.front[i];
    return list;
}
struct SlotHeap {                                   // when each of a class's slots is free next
    std::vector<double> h;
    explicit SlotHeap(int cap) : h((size_t)std::max(cap, 1), 0.0) {}
    double top() const { return h.front(); }
    double second() const { return h.size() < 2 ? 1e300 : h.size() < 3 ? h[1] : std::min(h[1], h[2]); }      // when the next one frees once the first is taken
    void replace_top(double v) { std::pop_heap(h.begin(), h.end(), std::greater<double>()); h.back() = v; std::push_heap(h.begin(), h.end(), std::greater<double>()); }
};
}  // namespace

double up_makespan(const std::vector<int> &list, const int *parent, const int *nsb, int nF, int cap) {
    const UpTree T(list, parent, nsb, nF);
    std::vector<SlotHeap> slots(UP_NX, SlotHeap(cap));
    std::vector<double> last(UP_NX, 0.0), end(T.n, -1.0);
    double span = 0.0;
    for (int i = 0; i < T.n; i++) {                 // (entries in the order of their ids)
        const int c = T.cls[i];
        const double start = std::max(last[c], slots[c].top());
        double kids = -1.0;
        for (int k = T.first_kid[i]; k >= 0; k = T.next_kid[k]) { if (end[k] < 0) return -1.0; kids = std::max(kids, end[k]); }
        end[i] = T.first_kid[i] >= 0 ? std::max(start + UP_LEAD, kids) + T.cost[i] : start + T.cost[i];
        last[c] = start; slots[c].replace_top(end[i]); span = std::max(span, end[i]);
    }
    return span;
}

std::vector<int> up_schedule(const std::vector<int> &base, const int *parent, const int *nsb, int nF, int cap, int mode) {
    const UpTree T(base, parent, nsb, nF);
    if (mode < 2 || T.n == 0 || T.n > 20000) return base;
    std::vector<int> seq;
    seq.reserve(T.n);
    if (mode == 2) {
        // descending priority: a child's path is longer than its parent's by its own cost, so every child comes first
        for (int i = 0; i < T.n; i++) seq.push_back(i);
        std::stable_sort(seq.begin(), seq.end(), [&](int a, int b) { return T.prio[a] > T.prio[b]; });
    } else {
        // list schedule on the slot model: a front is emitted at the clock when its class has a free slot, a front with children not before its
        // last child's end minus the lead (it would only hold the slot and spin) -- unless the class frees no other slot before that time;
        // highest priority first; nothing to emit: the clock advances
        std::vector<SlotHeap> slots(UP_NX, SlotHeap(cap));
        std::vector<int> left(T.n, 0), ready, dep(T.n, -1), cur(UP_NX, 0);      // (dep, cur: up_slots' rule run alongside, for the ids so far)
        std::vector<double> kids_end(T.n, 0.0);
        for (int i = 0; i < T.n; i++) { for (int k = T.first_kid[i]; k >= 0; k = T.next_kid[k]) left[i]++; if (!left[i]) ready.push_back(i); }
        double clock = 0.0;
        while ((int)seq.size() < T.n) {
            int pick = -1; size_t where = 0;
            bool pick_due = false;
            double next = 1e300;
            for (size_t r = 0; r < ready.size(); r++) {
                const int i = ready[r], c = T.cls[i];
                const SlotHeap &sl = slots[c];
                // a front with children whose class has handed out a round of slots since its last child: the model's clock is a model, the ids
                // are what the hardware follows -- it goes before anything else, no more than a round behind that child
                const bool due = T.first_kid[i] >= 0 && UP_NX * (cur[c] + 1) + c > dep[i] + UP_NX * std::max(cap, 1);
                double from = T.first_kid[i] >= 0 && !due ? kids_end[i] - UP_LEAD : 0.0;
                if (from > clock && sl.second() > from) from = clock;      // (no other slot of its class frees before then: this one, or its prelude lands on the path)
                from = std::max(from, sl.top());
                if (from > clock) { next = std::min(next, from); continue; }
                if (pick < 0 || (due && !pick_due) || (due == pick_due && (T.prio[i] > T.prio[pick] || (T.prio[i] == T.prio[pick] && i < pick)))) { pick = i; where = r; pick_due = due; }
            }
            if (pick < 0) { clock = next; continue; }
            const double end = T.first_kid[pick] >= 0 ? std::max(clock + UP_LEAD, kids_end[pick]) + T.cost[pick] : clock + T.cost[pick];
            const int c = T.cls[pick], need = dep[pick] + 1, k = std::max(cur[c], need > c ? (need - c + UP_NX - 1) / UP_NX : 0);
            cur[c] = k + 1;
            slots[c].replace_top(end);
            seq.push_back(pick);
            ready[where] = ready.back(); ready.pop_back();
            const int p = T.par[pick];
            if (p >= 0) { dep[p] = std::max(dep[p], UP_NX * k + c); kids_end[p] = std::max(kids_end[p], end); if (--left[p] == 0) ready.push_back(p); }
        }
    }
    std::vector<int> list = up_slots(T, seq);
    // never behind level order under the model (a list schedule carries no such promise of its own)
    if (up_makespan(list, parent, nsb, nF, cap) > up_makespan(base, parent, nsb, nF, cap)) return base;
    return list;
}

int up_schedule_check(const std::vector<int> &list, const std::vector<int> &base, const int *parent, int nF) {
    if (list.size() % UP_NX) return -1;
    std::vector<int> id((size_t)nF, -1), want((size_t)nF, -1);
    size_t n = 0, nb = 0;
    for (size_t b = 0; b < base.size(); b++) if (base[b] >= 0 && base[b] < nF) { want[base[b]] = (int)(b % UP_NX); nb++; }
    for (size_t b = 0; b < list.size(); b++) {
        const int t = list[b];
        if (t == -1) continue;
        if (t < 0 || t >= nF || id[t] >= 0 || want[t] < 0) return -2;            // exactly base's fronts, each once
        id[t] = (int)b; n++;
    }
    if (n != nb) return -2;
    for (int t = 0; t < nF; t++) {
        if (id[t] < 0) continue;
        if (id[t] % UP_NX != want[t]) return -3;                                // the class it was given
        const int p = parent[t];
        if (p >= 0 && id[p] >= 0 && id[t] >= id[p]) return -4;                   // every child below its parent
    }
    if (list.size() > (size_t)UP_NX * std::max<size_t>(n, 1)) return -5;         // the k-th front emitted lies in round k at the latest
    return 0;
}

// ---- owners of the extend-add's destination columns (plan.h: asm_owners) ----------------------------------------------------------------------
void asm_owners(int nbc, int nw, const int *kids, int n_kids, const int64_t *rows_ptr, const int *nub, const int *rel, int *owner) {
    std::vector<int> items((size_t)std::max(nbc, 0), 0), order, wave_of((size_t)std::max(nbc, 0), 0), load((size_t)std::max(nw, 1), 0);
    for (int k = 0; k < n_kids; k++) {
        const int c = kids[k];
        for (int jb = 0; jb < nub[c]; jb++) {
            const int b = rel[rows_ptr[c] + jb];
            if (b >= 0 && b < nbc) items[b] += asm_items(nub[c], jb);
        }
    }
    for (int b = 0; b < nbc; b++) if (items[b] > 0) order.push_back(b);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return items[a] > items[b]; });       // (stable: ties keep the lower column first)
    for (int b : order) {
        int w = 0;
        for (int v = 1; v < nw; v++) if (load[v] < load[w]) w = v;                                           // (ties: the lower wave)
        wave_of[b] = w; load[w] += items[b];
    }
    // never behind the modulo rule (longest-first is a heuristic and carries no such promise of its own): where it is, the front keeps b mod nw
    std::vector<int> mload((size_t)std::max(nw, 1), 0);
    for (int b = 0; b < nbc; b++) mload[b % std::max(nw, 1)] += items[b];
    if (*std::max_element(load.begin(), load.end()) > *std::max_element(mload.begin(), mload.end()))
        for (int b = 0; b < nbc; b++) wave_of[b] = b % nw;
    for (int k = 0; k < n_kids; k++) {
        const int c = kids[k];
        for (int jb = 0; jb < nub[c]; jb++) {
            const int b = rel[rows_ptr[c] + jb];
            owner[rows_ptr[c] + jb] = (b >= 0 && b < nbc) ? wave_of[b] : -1;
        }
    }
}

}  // namespace asam
