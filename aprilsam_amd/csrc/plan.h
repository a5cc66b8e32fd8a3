// plan.h — host-side symbolic plan of the multifrontal block-sparse Cholesky (MI355X-native design).
//
// The reference orders pose nodes with a constrained greedy min-degree (aprilsam.c:999-1249), hands
// the scalar matrix to CSparse's up-looking Cholesky in natural order (aprilsam.c:233-234) and keeps a
// block elimination tree (aprilsam.c:613-657).  Results do not depend on the ordering beyond ~1e-10
// (SURVEY.md §6), so this build uses its own: nested dissection on the pose graph, every separator and
// every leaf domain becoming one dense SUPERNODE ("front").  All indices below are in units of pose
// blocks (3 scalar unknowns each, aprilsam.c:141-148: idx = 3*position).
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

namespace asam {

struct Plan {
    int N = 0;                 // pose nodes
    int F = 0;                 // factors
    int leaf_nodes = 16;

    std::vector<int> perm;     // elimination position -> node id   (== param->ordering semantics)
    std::vector<int> pos;      // node id -> elimination position

    // ---- fronts, numbered in post-order (children before parents) ---------------------------------
    int nF = 0;
    std::vector<int> f_first;  // first own position; own blocks are positions [f_first, f_first+f_nsb)
    std::vector<int> f_nsb;    // # own (eliminated) blocks
    std::vector<int> f_nub;    // # update blocks (struct rows: positions > own, sorted ascending)
    std::vector<int> f_parent; // assembly-tree parent (front owning min struct position), -1 = root
    std::vector<int> f_level;  // 0 = no children; parent level = 1 + max(children)
    std::vector<int64_t> f_rows_ptr;  // CSR into f_rows / f_rel, size nF+1
    std::vector<int> f_rows;   // struct block positions of each front
    std::vector<int> f_rel;    // for each struct block: its block index inside the PARENT front's row list
                               //   (own blocks first: 0..nsb_p-1, then parent's struct blocks)
    std::vector<int> ch_ptr, ch_idx;   // children CSR (ascending front index)
    std::vector<int64_t> f_off;        // offset (doubles) of the frontal array in the HBM front pool
    int64_t pool_doubles = 0;

    // frontal array of front t: column-major, R = 3*(nsb+nub+1) rows (last block row = RHS row + 2 pad
    // rows), C = 3*(nsb+nub) columns, leading dimension R.  After factorisation columns [0,3*nsb) hold
    // L (L11 over L21 over the solved RHS row y), the trailing block holds the Schur update.
    inline int rows(int t) const { return 3 * (f_nsb[t] + f_nub[t] + 1); }
    inline int cols(int t) const { return 3 * (f_nsb[t] + f_nub[t]); }

    // ---- factor -> front assignment -------------------------------------------------------------------
    std::vector<int> fac_front;       // owner front (front of the earliest-eliminated node of the factor)
    std::vector<int> fac_la, fac_lb;  // local block index of node a / b in the owner front (lb=-1 unary)
    // gather lists: destination 3x3 blocks of every front and the factor contributions landing there.
    // block destinations (lower triangle incl. diagonal blocks):
    std::vector<int> bd_front_ptr;    // per front: range of block destinations, size nF+1
    std::vector<int> bd_row, bd_col;  // local block row / col (row >= col)
    std::vector<int> bd_src_ptr;      // CSR into bd_src, size nBD+1
    std::vector<int> bd_src;          // contribution id = 3*factor + {0: (a,a), 1: off-diagonal, 2: (b,b)}
    // rhs destinations:
    std::vector<int> rd_front_ptr;    // per front: range of rhs destinations, size nF+1
    std::vector<int> rd_col;          // local block col
    std::vector<int> rd_src_ptr;      // CSR into rd_src
    std::vector<int> rd_src;          // contribution id = 2*factor + {0: g_a, 1: g_b}
    std::vector<uint8_t> fac_swap;    // 1 if the off-diagonal block must be stored transposed (la < lb)
    // the same lists flattened for the device: one record per destination block of a front, sorted by
    // (front, block col, block row) with brow = -1 for the rhs row; contributions are stored by the
    // linearise kernel in SLOT order (= destination order), so a front's inputs are one contiguous stream.
    struct DestRec { int brow, bcol, src_begin, src_end; };
    std::vector<int> dest_front_ptr;  // per front: range of DestRec, size nF+1
    std::vector<DestRec> dest;
    std::vector<int> slot_blk;        // 3 per factor: slot of (a,a), off-diagonal, (b,b) block (-1 if absent)
    std::vector<int> slot_rhs;        // 2 per factor: slot of g_a, g_b
    int n_slots = 0;

    // ---- level schedule ---------------------------------------------------------------------------------
    int nLevels = 0;
    std::vector<int> lev_ptr, lev_fronts;   // fronts of each level

    // ---- statistics -----------------------------------------------------------------------------------------
    int max_rows = 0;          // max over fronts of 3*(nsb+nub)
    int64_t nnzL = 0;          // scalar nnz of L incl. diagonal (dense fronts)
    double flops = 0;          // sum_j c_j^2
};

// Build ordering + symbolic plan.  factor_nodes: 2 ints per factor (second = -1 for unary factors).
// xy: optional 2 doubles per node (used only as a hint for geometric bisection; any values are valid).
void build_plan(Plan &P, int N, int F, const int *factor_nodes, const double *xy, int leaf_nodes);
void build_gather_lists(Plan &P);     // fills bd_* / rd_* (only the tests' host-side emulator reads them: derived on demand)

// ---- XCD placement of the batch step's latency-bound launches (option xcd_place) --------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (observed, not promised): ids b and b + 8 share an XCD and its L2, where a
// hand-over written with plain stores is read about 1.7 x faster than from another XCD.  A heavy-path decomposition of the fronts of
// the multi-level launches gives each front a class 0..7: a front takes the class of its costliest child (critical path of a cost
// model), so the tree's critical path stays in one class from leaf to root, and the other children start classes of their own,
// balanced by count and cost, at most `cap` fronts per class (what an XCD holds at once; spill to the next class).  A front of class
// c goes to workgroup id 8 k + c, empty slots hold -1 (the kernels return at once there).  Every dependency keeps a lower workgroup
// id -- up: children before parents, down: parents before children -- the invariant that keeps the flag waits deadlock-free.  Leaves
// (the level-0 launch before the multi-level one) take their parent's class, at most cap_leaf per class.  Speed only: no result
// depends on where a workgroup runs.
struct XcdLists { std::vector<int> up, dn, leaf; };
// up: the fronts of the multi-level launches, children before parents; leaves: the fronts of the launch before them (may be empty)
XcdLists xcd_place(const std::vector<int> &up, const std::vector<int> &leaves, const int *parent, const int *nsb, int nF, int cap, int cap_leaf);
// 0, or a negative code naming the first violated invariant (permutation plus padding, dependencies at lower ids, classes within cap)
int xcd_check(const XcdLists &x, const std::vector<int> &up, const std::vector<int> &leaves, const int *parent, int nF, int cap, int cap_leaf);
// The back substitution's list when level 0 joins its multi-level launch (option persist_leaves): `dn` (parents first: XcdLists::dn, or the
// level-ordered list) followed by `leaf` (XcdLists::leaf, or level 0's list).  The upper fronts keep their workgroup ids, and -- both placed lists
// being whole multiples of 8 slots -- every leaf keeps the class it has in its own list, beside its parent's.
std::vector<int> dn_with_leaves(const std::vector<int> &dn, const std::vector<int> &leaf);
// 0, or a negative code: `list` is dn's slots unchanged, then exactly leaf's fronts, every parent at a lower id, (placed) classes as in dn / leaf
int dn_with_leaves_check(const std::vector<int> &list, const std::vector<int> &dn, const std::vector<int> &leaf, const int *parent, int nF, bool placed);

// ---- the order of the up-sweep's launch once level 0 is inside it (option persist_up) ---------------------------------------------------
// Dispatch follows the workgroup ids, so the ids are the schedule.  `base`: the launch's list in level order, children before parents, -1 in
// empty slots; a front's class is its slot % 8 there and stays (one class per front in both sweeps).  mode 2: descending priority, a front's
// priority being its remaining path to the root's end under the cost model (12 us + 0.19 us per own column with children, 4.8 us without).
// mode 3: a list schedule on the slot model -- `cap` slots per class, a class's ids dispatched in order as its slots free, a front holding its
// slot from dispatch to end, running its 4.3 us prelude at once and going on when its last child has ended; a front with children is emitted
// no earlier than its last child's end minus that prelude, highest priority first.  Either order is turned into ids by xcd_place's rule (the
// next id of the class above the class's last and above every child's), so every child keeps a lower id than its parent; the list is at most
// 8 n slots long for n fronts.  Where the model's makespan of the result exceeds that of `base`, `base` is returned.
std::vector<int> up_schedule(const std::vector<int> &base, const int *parent, const int *nsb, int nF, int cap, int mode);
// 0, or a negative code: whole rounds of 8 (-1), base's fronts each once (-2) in base's classes (-3), children at lower ids (-4), at most 8 n slots (-5)
int up_schedule_check(const std::vector<int> &list, const std::vector<int> &base, const int *parent, int nF);
// the model's makespan (us) of any such list, -1 where a child does not precede its parent
double up_makespan(const std::vector<int> &list, const int *parent, const int *nsb, int nF, int cap);

// ---- owners of the extend-add's destination columns (option asm_balance) -----------------------------------------------------------------
// A front's extend-add gives every destination block column to ONE wave of the workgroup, which adds every child's contribution to it, child
// after child: the order of each sum is fixed whoever the owner is, and the time behind the wait for the children is set by the wave with the
// longest work list.  Column b mod nw leaves the lists uneven; here the columns of ONE parent (nbc of them, `kids` its children) are taken by
// decreasing item count and each goes to the least loaded of the nw waves -- ties to the lower column, then to the lower wave.  An item is what
// the kernel's fill loop queues (asm_items: one per child block, one more where the block has a second 64-row pass).  owner[e] for every entry e
// of the children's block maps (the index of `rel`, rows_ptr[child] + block), -1 for an entry that maps outside the parent.  A parent whose
// longest list would come out longer than under b mod nw keeps b mod nw.
inline int asm_items(int cnu, int jb) { return 1 + (3 * cnu + 1 - 3 * jb > 64 ? 1 : 0); }
void asm_owners(int nbc, int nw, const int *kids, int n_kids, const int64_t *rows_ptr, const int *nub, const int *rel, int *owner);

// ---- pieces, exposed for tests --------------------------------------------------------------------------
struct NDTree {
    struct Node { std::vector<int> verts; std::vector<int> children; };
    std::vector<Node> nodes;
    std::vector<int> roots;
};
void nested_dissection(int N, const std::vector<int> &adj_ptr, const std::vector<int> &adj,
                       const double *xy, int leaf_nodes, NDTree &tree);

// ---- the planner's thread pool (ordering.cpp), for the other phases of a plan ------------------------------
// PlanSession: the pool's workers stay awake (polling) while one exists; for graphs below `min_nodes` nodes it does nothing and
// plan_parallel_for runs on the calling thread.  plan_parallel_for: body(begin, end) over disjoint chunks of [0, n), each of
// at least `grain` items; the chunks write disjoint outputs, so the result does not depend on the number of threads.
struct PlanSession { explicit PlanSession(int n_nodes, int min_nodes = 1024); ~PlanSession(); PlanSession(const PlanSession &) = delete; bool on = false; };
void plan_parallel_for(int n, int grain, const std::function<void(int, int)> &body);

}  // namespace asam
