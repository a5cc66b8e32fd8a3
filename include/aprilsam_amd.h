/* aprilsam_amd.h — C-ABI of libaprilsam_amd.so: the MI355X-native replacement for AprilSAM's
 * Gauss-Newton hot path (april_graph_cholesky / april_graph_cholesky_inc).
 *
 * The reference host program keeps compiling against its own aprilsam/aprilsam.h and simply links
 * (or dlopens) this library instead of libaprilsam.so for the symbols declared in PART 2.  PART 1
 * restates — from the measured LP64 layout, SURVEY.md §8(b) — the structs that cross the boundary,
 * so that this library, its tests and its Python mirror agree byte-for-byte with objects created by
 * reference-compiled code.  Nothing here carries torch or HIP types: plain pointers and sizes only.
 *
 * Citations are relative to the reference tree (xipengwang/AprilSAM @ v1).
 */
#ifndef APRILSAM_AMD_H
#define APRILSAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * PART 1 — boundary structs (layout-compatible restatements)
 * ---------------------------------------------------------------------------------------------- */

/* common/zarray.h:44-51 — 24 bytes; graph->nodes / graph->factors hold POINTERS as elements. */
typedef struct zarray {
    size_t el_sz;
    int    size;
    int    alloc;
    char  *data;
} zarray_t;

/* common/matd.h:46-51 — row-major dense matrix with a flexible data tail. */
typedef struct matd {
    unsigned int nrows, ncols;
    double       data[];
} matd_t;

/* aprilsam.h:65-72 — 32 bytes. attr/stype are opaque to the hot path. */
typedef struct april_graph {
    zarray_t   *factors;   /* elements: april_graph_factor_t*  */
    zarray_t   *nodes;     /* elements: april_graph_node_t*    */
    void       *attr;
    const void *stype;
} april_graph_t;

/* aprilsam.h:75-89 — result of a factor->eval() call (only produced by the host-side vtable
 * entries this library installs on the objects IT creates; the device path never builds one). */
typedef struct april_graph_factor_eval {
    double   chi2;
    matd_t **jacobians;   /* NULL-terminated, one per connected node */
    int      length;
    double  *r;
    matd_t  *W;
} april_graph_factor_eval_t;

#define APRIL_GRAPH_FACTOR_XYT_TYPE    1     /* aprilsam.h:91 */
#define APRIL_GRAPH_FACTOR_XYTPOS_TYPE 2     /* aprilsam.h:92 */
#define APRIL_GRAPH_NODE_XYT_TYPE      100   /* aprilsam.h:94 */

typedef struct april_graph_factor april_graph_factor_t;
typedef struct april_graph_node   april_graph_node_t;

/* aprilsam.h:98-146 — 104 bytes. The device path recognises type 1 (xyt) and 2 (xytpos) and reads
 * nodes[], u.common.z and u.common.W directly; function pointers are never called on the device.
 * This library's own max-mixture factors (type 3, u.max, PART 4) are native too.
 * Any other type (1 or 2 nodes) is evaluated on the HOST through ->eval(), as aprilsam.c:156 does. */
struct april_graph_factor {
    int   type;
    int   nnodes;
    int  *nodes;
    int   length;
    void *attr;
    april_graph_factor_t      *(*copy)(april_graph_factor_t *factor);
    april_graph_factor_eval_t *(*eval)(april_graph_factor_t *factor, april_graph_t *graph,
                                       april_graph_factor_eval_t *eval);
    april_graph_factor_eval_t *(*state_eval)(april_graph_factor_t *factor, april_graph_t *graph,
                                             april_graph_factor_eval_t *eval);
    void (*destroy)(april_graph_factor_t *factor);
    union {
        struct { double *z; double *ztruth; matd_t *W; void *impl; } common;
        struct { april_graph_factor_t **factors; double *logw; int nfactors; } max;
        struct { void *impl; } impl;
    } u;
    const void *stype;
};

/* aprilsam.h:151-179 — 112 bytes. */
struct april_graph_node {
    int     UID;
    int     type;
    int     length;
    double *state;
    double *init;
    double *truth;
    double *l_point;
    double *delta_X;
    void   *attr;
    april_graph_node_t *(*copy)(april_graph_node_t *node);
    void (*update)(april_graph_node_t *node, double *dstate);
    void (*relinearize)(april_graph_node_t *node);
    void (*destroy)(april_graph_node_t *node);
    void       *impl;
    const void *stype;
};

/* aprilsam.h:231-265 — 128 bytes.  chol / A / tr are the reference's CPU solver state; this library
 * keeps its (device) solver state in a side context keyed by the param pointer and leaves those
 * three NULL, so a reference-compiled april_graph_cholesky_param_destory() stays safe. `ordering`
 * is always a malloc() block (or NULL); factor_num / nreordering / batch_time keep their meaning. */
typedef struct april_graph_cholesky_param {
    double  tikhanov;      /* lambda added to every diagonal in a batch step (default 1e-4) */
    void   *chol;          /* unused here (NULL) */
    int     factor_num;    /* #factors folded into the current factorisation */
    int    *ordering;      /* position -> node id of the current elimination order */
    int     nreordering;   /* #nodes in the current factorisation; must be non-zero on entry */
    int     show_timing;
    double *delta_x;       /* kept only if pre-allocated by the caller (aprilsam.c:363-366) */
    double *B;             /* unused here (NULL) */
    double *y;             /* unused here (NULL) */
    void   *A;             /* unused here (NULL) */
    void   *tr;            /* unused here (NULL) */
    double  l_thresh;
    double  delta_thresh;
    int     nthreshold;
    double  batch_time;
    double  delta_xy;
    double  delta_theta;
} april_graph_cholesky_param_t;

/* ------------------------------------------------------------------------------------------------
 * PART 2 — the drop-in entry points (same names, arguments and error behaviour as the reference)
 * ---------------------------------------------------------------------------------------------- */

/* replaces aprilsam.c:33-39 (aprilsam.h:44): the banner the reference's example programs print first */
void APRILSAM_VERSION(void);
/* replaces aprilsam.c:45-64 */
void april_graph_cholesky_param_init(april_graph_cholesky_param_t *param);
/* replaces aprilsam.c:66-85 (frees the side context, the owned arrays AND param itself) */
void april_graph_cholesky_param_destory(april_graph_cholesky_param_t *param);
/* replaces aprilsam.c:87-375 — one batch Gauss-Newton step on the GPU; synchronous: every
 * node->state / l_point / delta_X is valid in host memory on return. Silent no-op on an empty graph. */
void april_graph_cholesky(april_graph_t *graph, april_graph_cholesky_param_t *param);
/* replaces aprilsam.c:377-576 — incremental step (new nodes/factors since the last call). */
void april_graph_cholesky_inc(april_graph_t *graph, april_graph_cholesky_param_t *param);
/* replaces aprilsam.c:578-597 — solve + state update of the current incremental factorisation. */
void april_graph_cholesky_inc_solver(april_graph_t *graph, april_graph_cholesky_param_t *param, int *idxs);
/* replaces april_graph.c:79-98 — chi^2 with the reference's 1/2-on-xyt-only convention (GPU). */
double april_graph_chi2(april_graph_t *graph);

/* ------------------------------------------------------------------------------------------------
 * PART 3 — host-side object constructors with the reference's names and ABI, so a caller (or a
 * test) can build a graph without the reference library.  replaces april_graph.c:329-364,
 * april_graph_xyt.c:276-298,420-438, april_graph_xytpos.c:191-211, april_graph.c:33-49.
 * ---------------------------------------------------------------------------------------------- */
april_graph_t *april_graph_create(void);
void           april_graph_destroy(april_graph_t *graph);
april_graph_node_t   *april_graph_node_xyt_create(const double *state, const double *init, const double *truth);
april_graph_factor_t *april_graph_factor_xyt_create(int a, int b, const double *z, const double *ztruth, const matd_t *W);
april_graph_factor_t *april_graph_factor_xytpos_create(int a, double *z, double *ztruth, matd_t *W);
void april_graph_factor_eval_destroy(april_graph_factor_eval_t *eval);
int  april_graph_dof(april_graph_t *graph);
/* `.graph` files: replaces april_graph_save / april_graph_create_from_file
 * (april_graph.c:377-426) and the object stream under them (common/stype.c:75-169, encode_bytes.h:120-250) for xyt
 * nodes and xyt / xytpos factors.  save returns 1 on success, 0 on failure (the reference's convention); load
 * returns NULL on failure.  String attributes survive a round trip (see aprilsam_amd_attr_*); attribute values of
 * other types are skipped on input. */
int            april_graph_save(april_graph_t *graph, const char *path);
april_graph_t *april_graph_create_from_file(const char *path);
void           april_graph_stype_init(void);      /* april_graph.c:367-375; nothing to register here */

/* ------------------------------------------------------------------------------------------------
 * PART 4 — extensions (prefix aprilsam_amd_). Not part of the reference API.
 * ---------------------------------------------------------------------------------------------- */

/* zarray_add is `static inline` in the reference (common/zarray.h:180-189), so it is not an
 * exported symbol there either; these two do the same append for callers without that header. */
void aprilsam_amd_graph_add_node(april_graph_t *graph, april_graph_node_t *node);
void aprilsam_amd_graph_add_factor(april_graph_t *graph, april_graph_factor_t *factor);

/* String attributes (the only kind the `.graph` files of the path carry: "type" = "odom" | "scan" on the demo's
 * factors, examples/aprilsam_demo.c:84-86; reference API: april_graph_*_attr_put/get, april_graph.c:101-176).
 * attr_slot is &node->attr, &factor->attr or &graph->attr of an object created by THIS library; a slot already
 * holding the reference library's attribute table is refused (-2).  Objects' copy()/destroy() carry them along. */
int         aprilsam_amd_attr_put_string(void **attr_slot, const char *key, const char *value);
const char *aprilsam_amd_attr_get_string(const void *attr, const char *key);
int         aprilsam_amd_attr_count(const void *attr);
int         aprilsam_amd_attr_item(const void *attr, int i, const char **key, const char **value);

/* Same as april_graph_save / april_graph_create_from_file.  save_ex starts the per-object magic counter of the file
 * format `magic_offset` objects later, which reproduces byte for byte what a reference process writes after it has
 * already encoded that many objects (csrc/graph_io.cpp; data/M3500.graph: 8 * 5453). */
int            aprilsam_amd_graph_save(april_graph_t *graph, const char *path);
int            aprilsam_amd_graph_save_ex(april_graph_t *graph, const char *path, unsigned long long magic_offset);
april_graph_t *aprilsam_amd_graph_load(const char *path);

/* Host-only consistency checks of the index arithmetic shared by launch tables and kernels (tile decode of the
 * outer-blocked trailing update, packed Schur offsets, panel row tiles, LDS budgets).  0 = all good.  No GPU needed. */
int aprilsam_amd_selftest(void);

/* Number of usable HIP devices (0 => every solver entry point fails loudly: error -14, see below). */
int aprilsam_amd_device_count(void);
/* Select the HIP device used by contexts created afterwards (default: LOCAL_RANK env or 0). */
int aprilsam_amd_set_device(int device);
/* Bind ONE param (and the graph it is called with) to a device slot, 0 <= slot < 64: slot s runs on HIP device s % device_count, so on a
 * node with N devices the slots 0 .. N-1 are the devices and further slots share them.  Calls on params bound to different slots run
 * concurrently from different threads (each slot has its own lock, every call makes its slot's device current on the calling thread):
 * one C process can drive N solves on N devices without forking -- the reference's solver has no process-wide state either (SURVEY
 * section 8(b) "Threading").  Calls on the same slot are serialised.  Whatever the param held (plan, fronts, captured graphs) is dropped;
 * a graph's device copies follow the slot of the param it is called with (one graph is driven from one slot at a time).  Options
 * (aprilsam_amd_set_option) stay process-global: set them while no call is in flight.  Returns 0, -1 for a bad slot.
 * The binding lasts until april_graph_cholesky_param_init or _destory of that param (bind AFTER _init, as the example in
 * INTEGRATION.md section 4b does): a param allocated later at the same address starts on the default slot.
 * aprilsam_amd_param_get_device: the HIP device a call on this param runs on. */
int aprilsam_amd_param_set_device(const april_graph_cholesky_param_t *param, int slot);
int aprilsam_amd_param_get_device(const april_graph_cholesky_param_t *param);

/* Per-param solver statistics of the LAST solver call (all times in milliseconds).  */
typedef struct aprilsam_amd_stats {
    int    n_nodes, n_factors;
    int    n_fronts, n_levels;         /* supernodal assembly tree */
    int    max_front_rows;             /* largest frontal dimension (scalar rows, w/o rhs row) */
    int    symbolic_reused;            /* 1 if ordering+symbolic came from the cache */
    int    not_spd;                    /* 1 if a non-positive pivot was met (states left untouched) */
    int    reserved0;
    long long nnz_L;                   /* scalar non-zeros of L incl. diagonal (dense-front count) */
    double flops_factor;               /* sum_j c_j^2 of our own L (SURVEY §8(d) convention) */
    double bytes_fronts;               /* bytes of all frontal matrices resident in HBM */
    double ms_pack, ms_symbolic, ms_h2d, ms_device, ms_d2h, ms_unpack, ms_total;
    double ms_dev_linearize, ms_dev_factor, ms_dev_solve;   /* HIP-event timings inside ms_device */
    double chi2_before;                /* chi^2 at the linearisation point (from the linearise kernel) */
    int    error_code;                 /* 0, or the code of the failure that ended the last call on this param (see below) */
    int    reserved1;          /* 1: a warm batch call launched on the packed factor copies, found an edited factor object afterwards and ran again (speculate_factors) */
    /* last april_graph_cholesky_inc on this param (both 0 after any other call): */
    int    inc_replanned;      /* 1: the step did not fit the frozen plan of the last batch step and was solved on a fresh plan (ordering +
                                  symbolic analysis + every front factorised); the result is the exact solve of the incremental system */
    int    inc_old_old_cross;  /* number of the step's new factors that connect two poses which BOTH predate the call and lie in different
                                  branches of the reference's elimination tree.  For those the reference's partial re-factorisation
                                  (aprilsam.c:850-906, children first over the OLD tree) finalises one row before the other has updated it and
                                  returns something that is NOT the solution of its own normal equations; this library returns the exact solve
                                  (INTEGRATION.md section 4).  > 0 therefore means: this step's states deviate from the reference's by design */
    int    inc_fronts_updated; /* fronts whose factor took a low-rank update in this step (option "inc_update") instead of being re-assembled and
                                  re-factorised; reserved0 counts all fronts the step regenerated */
    int    dn_launch_fronts;   /* fronts in the step's multi-level back substitution launch (one workgroup each, x handed from parent to child inside the launch), 0: none */
    int    up_launch_fronts;   /* fronts in the batch step's multi-level factorisation launch (level 0 included where option "persist_up" joined it), 0: none */
} aprilsam_amd_stats_t;
int aprilsam_amd_get_stats(const april_graph_cholesky_param_t *param, aprilsam_amd_stats_t *out);

/* Failure path.  The reference's entry points are void and crash on bad input (assert / NULL dereference, SURVEY.md
 * section 8(b)); this library never takes the caller's process down.  A call that fails returns with the caller's node states
 * untouched, prints one line on stderr, and leaves
 *     -2  a pivot was not positive (stats.not_spd = 1; information matrix not positive definite)
 *     -9  a multi-level launch gave up waiting for a dependency flag (should not happen; reported, not hung)
 *    -10  a HIP runtime call failed                  -11  device / pinned memory exhausted (or option "mem_cap_mb")
 *    -12  unsupported input: node type other than xyt, a foreign factor (own eval()) with more than 11 nodes, a factor of a native type
 *         with the wrong number of nodes, an unsplittable dense region of
 *         more than ~6000 poses, more than 22 million factors, param->nreordering == 0 (the reference asserts)
 *    -13  malformed graph: node index out of range, a factor connecting a node to itself, incomplete eval() result
 *    -14  no HIP device visible: there is NO CPU fallback, every solver call on such a machine fails this way (april_graph_chi2
 *         returns NaN) -- nothing is ever computed on the host
 *    -15  internal inconsistency of the planner
 *    -16  debug option "pool_guard": a kernel wrote into the guard band behind a frontal array
 * in stats.error_code and in aprilsam_amd_last_error (most recent failure of the process; msg may be NULL).  For every code but -2
 * the param's cached plan and factorisation are dropped: the next april_graph_cholesky starts from scratch, april_graph_cholesky_inc
 * returns silently until then (no prior factorisation, aprilsam.c:382-383).  After -2 only the factorisation goes (next paragraph).
 * stats.not_spd and stats.error_code speak for the most recent solver call on the param: a call that succeeds resets both.
 *
 * What -2 leaves behind, per entry point.  The numeric phase stopped with fronts half written, so the param's
 * FACTORISATION is dropped whatever it held before -- april_graph_cholesky_inc and april_graph_cholesky_inc_solver return silently, the
 * covariance / gating / solve entry points return -1 and write nothing, aprilsam_amd_factorised_nodes returns -1 -- until an
 * april_graph_cholesky succeeded; the PLAN is kept (it describes the graph, not the numbers), and a repaired graph gives the bits of a
 * fresh graph and param.  param->ordering, nreordering, factor_num and delta_x are not written.
 *   april_graph_cholesky        every node's state and delta_X untouched; l_point = state and UID = index ARE written, as the reference
 *                               writes them before it factorises (aprilsam.c:131-135, 628)
 *   april_graph_cholesky_inc    states, delta_X, l_points and UIDs untouched
 *   aprilsam_amd_resident_*     sync returns -2; end returns -2 and writes nothing at all: the node objects stay as resident_begin found them,
 *                               also where the failed step moved the device states of a healthy component of the graph (with or without
 *                               a resident_sync before it).  A loop that ran no step records no factorisation: begin / end after a
 *                               failed call leaves the param without one
 *   aprilsam_amd_optimize_lm    the step is rejected and counted in rejected_not_spd (see there); not a failure of the call */
int  aprilsam_amd_last_error(char *msg, int cap);
void aprilsam_amd_clear_error(void);

/* Runtime options (also settable by env APRILSAM_AMD_<NAME>): returns 0 on success.
 *   "leaf_nodes"        nested-dissection leaf size in pose nodes (default 16)
 *   "deterministic"     1 = disable the wall-clock fallback rule aprilsam.c:557-559; default 0 = the reference's behaviour: an incremental step
 *                       that took longer than param->batch_time / 3 falls back to a batch step, so the schedule of fall-backs (and with it
 *                       the states, within the solver's tolerance) depends on the machine's timing exactly as the reference's does.  Parity
 *                       runs and recorded schedules set 1 (env APRILSAM_AMD_DETERMINISTIC=1)
 *   "use_graph"         1 = replay the numeric phase from a captured hipGraph (default 1)
 *   "device_timing"     1 = record per-stage HIP events (default 0)
 *   "trust_factor_cache" 1 = z/W of already-packed factors are treated as immutable: skips the per-call re-read and
 *                       comparison of every factor object (default 0: reference semantics, edits in place are seen)
 *   "small_lds_kb"      LDS budget (KiB) of the single-workgroup front kernel: fronts whose whole array fits run fully
 *                       in LDS, fronts whose own columns fit run in panel mode, the rest takes the multi-workgroup
 *                       path (default 156; 0 forces the multi-workgroup path everywhere)
 *   "panel_mode"        0 = no panel mode (fronts that do not fit LDS entirely go to the multi-workgroup path) (1)
 *   "tp_fronts", "tp_lds_kb"  levels with at least tp_fronts fronts (default 1000) are throughput-bound: there only
 *                       fronts up to tp_lds_kb KiB (default 80: two workgroups per compute unit) run fully in LDS, larger ones use panel mode so that
 *                       several workgroups share a compute unit
 *   "small_threads", "tp_threads"  workgroup size of the single-workgroup front kernel (256 / 512 / 1024) on
 *                       latency-bound levels (default 1024) and on throughput levels (default 512)
 *   "schur_first"       small fronts in panel mode with at least this many update blocks store the Schur product into their update
 *                       columns first and add the factor blocks / children's update blocks afterwards (no zero fill, no atomics
 *                       for the product); default 40, 0 = never
 *   "syrk_small_tiles"  wide trailing updates of fewer 64x64 tiles than this use 32x32 tiles (four times the workgroups, a quarter of
 *                       the K loop each); default 320 = a quarter of a round of workgroups, 0 = never
 *   "syrk_pair_tiles", "syrk_group"  multi-workgroup fronts on levels whose first wide update has at least syrk_pair_tiles 64x64 tiles
 *                       (default 2048; 0 = never) close every GROUP of syrk_group outer blocks (default 3; 2 .. 8) with ONE wide update of
 *                       K = the group's columns instead of one per 128 columns: the far part of the trailing matrix is read and written once
 *                       per group; inside a group only the next block's own columns are updated (left-looking, K = the group so far)
 *   "syrk_xcd_order"    wide trailing updates of at least this many 64x64 tiles use the XCD-aware tile order (default 512 = one
 *                       round of workgroups; 0 = never, 1 = always)
 *   "batch_extend"      1 (default): april_graph_cholesky on a graph that only GREW since the last plan keeps the plan -- the
 *                       appended poses become tail fronts, every front is re-factorised (batch semantics) -- instead of a new
 *                       ordering + symbolic analysis per call; once more than "extend_tail_fronts" (default 3) x 24 poses have been
 *                       appended (the unit is fixed at 24 poses whatever "tail_poses" -- default 28 -- says), or when the topology stops
 *                       changing, a full re-plan follows.  0 = re-plan on every topology change
 *   "pin_last"          k > 0: the k newest poses are kept out of the nested dissection and form the root front ("recent
 *                       poses last", cf. aprilsam.c:1021-1098); default 0, measured effect in profiles/r02_inc_hist.json
 *   "speculate_factors" 1 (default): a warm april_graph_cholesky call on an unchanged graph launches the step on the packed factor
 *                       copies first and reads every factor object (z / W edited in place?) while the GPU works; an edit voids that
 *                       run and the call starts over (stats.reserved1 = 1).  0 = read the factor objects before launching
 *   "warm_up"           1 (default): the first april_graph_cholesky_param_init of a process initialises what the HIP runtime sets up
 *                       lazily -- two streams (8-20 ms each: a graph owns one), the copy engines' queues (7 ms per direction), the code object (2 ms), the graph
 *                       machinery (8 ms) -- so that those milliseconds do not land inside the first solver calls (or, for the first
 *                       device-to-host copy, inside an incremental step a thousand steps into a run).  Without a device it does
 *                       nothing.  0 (set APRILSAM_AMD_WARM_UP=0 in the environment: it is read before the first param exists) =
 *                       everything stays lazy.  Streams are recycled per device slot either way (a released graph parks its stream)
 *   "inc_fast"          0 = every incremental step re-plans (default 1: frozen base plan + dirty root paths)
 *   "inc_multi"         0 = incremental steps launch their fronts / back substitution level by level (default 1: one multi-level
 *                       launch per direction, fronts synchronised by dependency flags)
 *   "inc_one"           1 (default, needs inc_multi): an incremental step that regenerates at most "inc_one_up" (3) fronts and walks
 *                       at most "inc_one_dn" (4) runs as ONE launch of one workgroup of "inc_one_threads" (512) threads -- patches,
 *                       linearisation, fronts, back substitution, state update; "inc_one_spin" (1): its completion is a word in
 *                       pinned host memory the host spins on (0: hipStreamSynchronize)
 *   "inc_tail"          1 (default, needs inc_multi): steps whose new factors touch only the last 8 poses of the last tail front
 *                       re-factorise that front's trailing columns alone (the front keeps the shape of a full one through phantom
 *                       rows); 0 = every dirty front is re-assembled and re-factorised in full
 *   "inc_inline"        1 (default): a small step's patches (<= 24 ranges, <= 2 KiB) travel in the kernel arguments; 0 = always read
 *                       from pinned host memory by the kernel
 *   "inc_update"        1 (default, needs inc_multi): a new factor between an old pose and a recent one UPDATES the factor of every front
 *                       on the old pose's root path (three vectors per factor travelling up the assembly tree; the last tail front is
 *                       still re-factorised) instead of re-assembling and re-factorising those fronts; stats.inc_fronts_updated counts
 *                       them.  0 = round-3 behaviour
 *   "inc_tail_solve"    1 (default, needs inc_tail): when every pose the step's walk visits lies among the last 8 poses, the back
 *                       substitution and the state update run inside the same single-workgroup launch, on the trailing columns alone
 *   "inc_lazy_states"   1 (default): an incremental step whose walk is partial compares only the node objects it reads (the poses of its new
 *                       factors, the visited poses, the new poses) with the library's state mirrors; 0 = every node object on every step
 *   "inc_replan_tall"   1 (default): when a front of a plan made of single-workgroup fronts only has collected so many loop-closure rows that
 *                       it no longer fits the LDS, the step re-plans; 0 = it takes the multi-workgroup path from then on
 *   "tail_poses"        own poses per tail front of the incremental path (default 28, at least 8)
 *   "persist"           1 (default): the top levels of the elimination tree -- as many as hold at most "persist_max_fronts"
 *                       (default 240) single-workgroup fronts -- run as ONE launch per sweep, fronts synchronised by
 *                       per-front dependency flags that carry the step number and are never reset (round 5 found a release in these
 *                       launches that did not wait for its L2 write-back -- a wrong result about once in 10^4 solves of chain-like graphs,
 *                       profiles/r05_flag_soak.txt; the soak of the corrected build is profiles/r06_flag_soak.txt);
 *                       0 = one launch per level, no flags -- the conservative setting, M3500 then
 *                       costs about a quarter more per iteration (what the multi-level launches bought when they were introduced: 0.366 -> 0.294 ms)
 *   "xcd_place"         1 (default): the lists of those launches, and of the level-0 launches below them, are ordered so that a front
 *                       runs on the XCD of the child on its critical path (workgroups b and b + 8 share an XCD: observed, not promised);
 *                       speed only, results bitwise the same; 0 = level by level
 *   "persist_leaves"    1 (default): where only "persist_max_fronts" kept level 0 out of those launches -- level 0 holds single-workgroup
 *                       fronts only, the launch still fits the LDS with them, every front keeps its kernel -- the leaves run as the last
 *                       workgroups of the back substitution's launch and take x from their parents inside it (M3500: one launch of 680
 *                       fronts instead of 201 + 479); speed only, results bitwise the same; 0 = level 0 keeps its own launch
 *   "persist_up"        the factorisation's half of the same (APRILSAM_AMD_PERSIST_UP), under the same condition and only where no front changes
 *                       between its full-LDS and its panel form: 0 = level 0 keeps its own launch; 1 = level 0 inside the multi-level
 *                       launch, level order; 2 (default) = ... in descending order of the remaining path to the root under a cost model
 *                       (M3500: resident step 0.1981 -> 0.1877 ms); 3 = ... in
 *                       the order of a list schedule that knows how many workgroups an XCD holds at once (plan.h: up_schedule).  2 and 3 also
 *                       order the launch of graphs that run one launch per sweep anyway.  Speed only, results bitwise the same
 *   "asm_balance"       1 (default): in the extend-add of a single-workgroup front, the block columns are given to the workgroup's waves by
 *                       their number of work items, longest first to the least loaded wave (aprilsam_amd_asm_owners), so that no wave's
 *                       list is longer than it has to be; 0 = column modulo waves everywhere (APRILSAM_AMD_ASM_BALANCE).  One wave per column
 *                       either way, so every sum keeps its order: speed only, results bitwise the same
 *   "blk_backsolve"     1 (default): multi-workgroup fronts are back-substituted 128 columns at a time by a chain
 *                       workgroup + helper workgroups, with the inverse diagonal blocks the factorisation left behind; 0 = one
 *                       workgroup per front, 32 columns at a time
 *   "wave_backsolve"    1 (default): fronts whose L panel fits LDS (multi-level launch, latency-bound levels, incremental
 *                       steps) are back-substituted column-per-lane -- one in-register chain per 64 columns; 0 = the
 *                       per-32-column-block kernel everywhere
 *   "tagged_x"          how a front of a multi-level back substitution hands its x to its children (APRILSAM_AMD_TAGGED_X).  1 (default):
 *                       as epoch-tagged 16-byte granules that the children's lanes poll, no flag; a launch that holds a front of more
 *                       than 256 update rows takes form 2.  0 = x stored write-through, then a flag, no L2 write-back.  2 = plain x,
 *                       L2 write-back, flag: the form of every other hand-over.  Speed only, results bitwise the same
 *   "linearize_staged_min"  graphs with at least this many factors (default 32768) write the J^T W J blocks out through
 *                       LDS with coalesced stores; smaller ones store directly (one latency chain less)
 *   "mem_cap_mb"        > 0: any single device buffer above this size is refused as if the device were out of memory
 *                       (error -11); 0 = off (default).  For testing the failure path
 *   "pool_guard"        debug, > 0: every frontal array of a plan is followed by a guard band of this many doubles (rounded up to 32), filled
 *                       with NaN when the plan is uploaded and checked after every synchronised step: a kernel that wrote into one ends the
 *                       call with error -16, a kernel that READ from one and used the value turns the results into NaN -- instead of a fault
 *                       that depends on where the allocation ends.  0 = off (default)
 *   "amalg", "amalg_max"  1: separator fronts of the nested dissection take in child separators where a model of the critical path (hand-over per
 *                       front against pivot chain per column) says so, up to amalg_max own poses (default 64) -- fewer dependent levels, more flops.
 *                       Measured on M3500 in round 6: no gain (profiles/r06_experiments_not_kept.txt); 0 = off (default)
 *   "pool_poison"       debug, 1: before every step the UPDATE block of every front the step (re)factorises -- what its parent reads -- and the
 *                       solution at its own positions -- what its children read -- are filled with NaN.  A dependency wait of a multi-level
 *                       launch that passes early then produces NaN / "not positive definite" with certainty instead of the previous step's
 *                       numbers (which are the right ones whenever the previous step solved the same system: the mask that hid round 5's
 *                       release defect from everything but a soak).  Costs one extra pass over the fronts.  0 = off (default)
 *   "skip_flag_waits"   debug, 1: the fronts of the batch path's multi-level factorisation launch do NOT wait for their children -- the negative
 *                       control of "pool_poison" (the result must then come back NaN / not positive definite).  0 = off (default)
 *   "polar_on_host"     debug, 1: range / bearing / range-bearing factors are packed as host-evaluated foreign
 *                       factors through their own eval() instead of natively -- the A/B oracle of the native path.  0 = off (default) */
int aprilsam_amd_set_option(const char *name, double value);
/* debug, with option "pool_guard" on and after a step on this param: points the guard check at a band inside a live frontal array; returns
 * -16 (the check works), -1 when the param has no guarded plan.  The param's cached plan is dropped, as after any failure */
int aprilsam_amd_debug_guard_selftest(const april_graph_cholesky_param_t *param);
/* current value of an option (after the environment and any set_option call): 0, or -1 for an unknown name */
int aprilsam_amd_get_option(const char *name, double *value);

/* ---- device-resident benchmark/driver API: states stay in HBM between iterations -------------
 * aprilsam_amd_batch_resident() runs `iters` batch Gauss-Newton iterations back to back without
 * touching host node objects in between (states/l_points live in HBM), then writes the final states
 * back into the graph.  chi2_out (may be NULL) receives iters+1 values: chi^2 before the first
 * iteration and after each one.  ms_out (may be NULL) receives `iters` HIP-event durations of
 * the device work per iteration.  Returns 0 on success, <0 on failure (no device, not SPD, ...). */
int aprilsam_amd_batch_resident(april_graph_t *graph, april_graph_cholesky_param_t *param, int iters,
                                double *chi2_out, double *ms_out);

/* The same, in pieces (what bench.py times): begin = pack + plan + upload (states now resident in HBM);
 * steps(n, mode) enqueues n Gauss-Newton iterations on the solver's HIP stream — mode 0 asynchronously
 * (hipGraph replay), mode 1 with every kernel launch bracketed by a HIP event pair on that stream and a
 * synchronisation per iteration; sync waits and returns -2 if a pivot was not positive; chi2 evaluates
 * chi^2 of the resident states; end leaves the node objects as the same number of april_graph_cholesky calls would
 * (aprilsam.c:131-135, 311-315): state = the final state, l_point = the point the LAST step was linearised at,
 * delta_X = that step's dx -- the factorisation of that step is kept, so april_graph_cholesky_inc may follow. */
int    aprilsam_amd_resident_begin(april_graph_t *graph, april_graph_cholesky_param_t *param);
int    aprilsam_amd_resident_steps(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, int mode);
int    aprilsam_amd_resident_sync(april_graph_t *graph, april_graph_cholesky_param_t *param);
double aprilsam_amd_resident_chi2(april_graph_t *graph);
int    aprilsam_amd_resident_end(april_graph_t *graph, april_graph_cholesky_param_t *param);
/* Per-kernel totals of the mode-1 passes since resident_begin (ms, launches) and the ALGORITHMIC flops /
 * bytes one iteration asks of each kernel (SURVEY.md §8(d) conventions).  Arrays of 16; returns the
 * number of kernels filled; names[k] points at static strings. */
int aprilsam_amd_kernel_profile(const april_graph_cholesky_param_t *param, double *ms, long long *calls,
                                double *flops, double *bytes, const char **names);
/* The same passes per LEVEL of the assembly tree: out6[6 * l + ...] = {ms factorisation (assembly included), ms back substitution,
 * fronts, fronts on the multi-workgroup path, widest own part (scalar columns), sum c_j^2 flops of the level}; a multi-level
 * launch is booked on its first level.  Returns the number of levels (fills at most cap_levels). */
int aprilsam_amd_level_profile(const april_graph_cholesky_param_t *param, double *out6, int cap_levels);

/* ---- marginal covariances from the retained factor ---------------------------------------------------
 * Marginal covariances of the system the LAST successful solver call on `param` factorised: the inverse of
 * (sum J^T W J + diag(lambda)) at that step's linearisation points (the nodes' l_point after the call), read from the retained
 * factor by selected inversion on the GPU.  Available after april_graph_cholesky, aprilsam_amd_batch_resident,
 * aprilsam_amd_resident_end and april_graph_cholesky_inc (whichever way the step went: fast path with tail fronts, low-rank updates,
 * re-plan, batch fall-back).  lambda sits where the step put it: param->tikhanov on every pose after a batch call (an extended plan
 * included); after an incremental step on the positions that carry it in the factorised system (DevPlan::lambda): the poses present at
 * the last batch step.  Sigma is recomputed in full after every solver call.
 * nodes == NULL: all nodes (n ignored; the graph must hold exactly the factorised nodes).  cov: 9 doubles per node, row-major
 * (x, y, theta: the unknowns of delta_X).  Returns 0, or < 0:
 *   -1   no retained factor (never solved, the last solver call failed or was not positive definite, a resident run in progress)
 *        A resident run is in progress from aprilsam_amd_resident_begin to aprilsam_amd_resident_end, also before its first step.  A loop
 *        that ended without a step leaves the factor that begin found -- unless begin had to plan a changed graph (factors or nodes added
 *        since): the fronts were laid out anew, and the param is without a factor until its next successful solver call.  The same holds
 *        after an aprilsam_amd_debug_stage call that had to plan.  In both states april_graph_cholesky_inc and april_graph_cholesky_inc_solver
 *        return silently, as on a param without a factorisation.
 *   -12  sharded param; the factorised graph holds a factor with an asymmetric information matrix (the reference-order path
 *        factorises one triangle of an unsymmetric system: no covariance is defined)
 *   -13  a node id out of range of the factorised system (nodes added since the last solve), or a bad argument
 *   -14  no HIP device
 * It sets aprilsam_amd_last_error like every entry point, but -- unlike the solver entry points -- a failed marginals call leaves
 * the param's plan and factor in place: it only reads them, and the next solver call is unaffected.  Sigma is computed once per
 * factorisation and kept beside the factor (a second pool of stats.bytes_fronts bytes, allocated on the first call, freed with the
 * plan; option mem_cap_mb applies): a second call with no solver call in between only extracts.  Two calls give the same bits.
 * The system is the PARAM's: `graph` only sizes the nodes == NULL form here and, in aprilsam_amd_gate_xyt, aprilsam_amd_gate_polar and
 * aprilsam_amd_relative_covariances, supplies the CURRENT states.  After the param's last successful call was made with another graph, or
 * after the graph was destroyed and built again, these calls (and aprilsam_amd_marginals_joint / _joint_any / _marginals_cross /
 * aprilsam_amd_solve) still answer for the system that call factorised; only aprilsam_amd_factor_audit and aprilsam_amd_marginal_prior,
 * which read the graph's device copy, return -1.  A factor's z / W edited in place, or a factor added between old poses, is not seen
 * before the next solver call (or april_graph_chi2): every consumer keeps answering for the factorised system. */
int aprilsam_amd_marginals(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *nodes, double *cov);
/* Joint covariance [[S_aa S_ab]; [S_ba S_bb]] (36 doubles per pair, row-major, a's unknowns first) for pairs on the factor's
 * pattern -- every pair joined by a factor is.  Returns the number of pairs NOT on the pattern (their 36 values are NaN), or the
 * codes above. */
int aprilsam_amd_marginals_joint(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, double *cov);
/* debug: number of selected inversions run on this param so far (-1: no context) */
long long aprilsam_amd_debug_selinv_runs(const april_graph_cholesky_param_t *param);

/* ---- joint covariances of any pose pair, and gating of candidate measurements ---------------------------
 * Joint covariance [[S_aa S_ab]; [S_ba S_bb]] of ANY pairs (36 doubles per pair, row-major, a's unknowns first; a == b allowed), of the
 * same system as aprilsam_amd_marginals: the inverse of the system the last successful solver call on `param` factorised (lambda where
 * the step put it, evaluated at the nodes' l_point), read from the retained factor.  Every value is finite, whatever the pattern of L:
 * S_ab = (L^-1 E_a)' (L^-1 E_b) by triangular solves along the assembly-tree paths of the two poses on the GPU (no selected inversion
 * runs, no Sigma pool is allocated; the work buffer is chunked to at most 1 GB, or to option mem_cap_mb).  Returns 0, or the codes of
 * aprilsam_amd_marginals (-1 no retained factor or a resident run in progress; -12 sharded param or asymmetric W in the factorised graph;
 * -13 a node id out of range or a null argument; -14 no HIP device).  A failed call writes nothing and changes nothing.  Two calls give
 * the same bits.  aprilsam_amd_marginals_joint keeps its NaN for pairs off the pattern. */
int aprilsam_amd_marginals_joint_any(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, double *cov);
/* Mahalanobis gating of n candidate xyt measurements: z[3i..] (x, y, theta of b in a's frame) with information W[9i..] (row-major)
 * between nodes a[i] and b[i].  Per candidate, on the GPU right after the path solves:
 *     r, J_a, J_b   residual and Jacobians exactly as an xyt factor computes them (theta wrapped), at the nodes' CURRENT state
 *                   (what graph holds now: after a solver call, the updated states)
 *     S  = [J_a J_b] Sigma_ab [J_a J_b]' + W^-1     Sigma_ab: aprilsam_amd_marginals_joint_any's block, i.e. at the l_points of the
 *                                                  last solver call
 *     d2 = r' S^-1 r      (compare with a chi^2 quantile of 3 degrees of freedom: 16.27 at 0.999)
 * d2: n doubles; S: 9 n doubles (row-major) or NULL.  Returns 0, or the codes above, and: -12 a W that is not symmetric (mirror entries
 * bitwise equal) positive definite; -13 a == b, a non-finite z or W, a node id out of range of the factorised system or of graph, a null
 * argument.  Nothing is written on a refusal. */
int aprilsam_amd_gate_xyt(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, const double *z,
                          const double *W, double *d2, double *S);
/* ---- node sets and joint compatibility of closure hypotheses ----------------------------------------------------
 * aprilsam_amd_marginals_set: the dense joint covariance of the k listed nodes, cov (3k) x (3k) row-major, node i's unknowns at rows /
 * columns 3i..3i+2, of the same system as aprilsam_amd_marginals_joint_any.  Any k >= 0 (k == 0 returns 0 and writes nothing); a node may
 * be listed more than once, its blocks repeat.  Every distinct node is solved once, every distinct unordered pair goes through the path
 * solves' block kernel once (work buffer chunked as for _joint_any): block (i, j) equals _joint_any's S_ab of the pair (nodes[i], nodes[j])
 * bit for bit, the matrix is exactly symmetric, blocks across the components of a disconnected graph are exactly 0.0, the rows and columns
 * of a fixed node are exact zeros.  Returns 0 or _joint_any's codes; -11 when a buffer does not fit under option mem_cap_mb.
 *
 * aprilsam_amd_gate_xyt_joint: the joint compatibility test (Neira and Tardos) of n_hyp hypotheses, each a list of 1 .. APRILSAM_AMD_JOINT_MAX
 * candidate xyt measurements as aprilsam_amd_gate_xyt takes them; hyp_ptr (n_hyp + 1 entries, hyp_ptr[0] == 0, CSR) indexes a / b / z / W.
 * Per hypothesis with candidates i = 0 .. m - 1, on the GPU behind the path solves:
 *     r_i, J_ai, J_bi    exactly as aprilsam_amd_gate_xyt: residual (theta wrapped) and Jacobians at the nodes' CURRENT states
 *     C = H Sigma_set H' + blockdiag(W_i^-1)     (3m x 3m; H holds J_ai, J_bi in the columns of a_i, b_i; Sigma_set: the joint covariance
 *                        of the hypothesis's distinct nodes, at the l_points of the last solver call).  Block (i, j) =
 *                        J_ai S(a_i,a_j) J_aj' + J_ai S(a_i,b_j) J_bj' + J_bi S(b_i,a_j) J_aj' + J_bi S(b_i,b_j) J_bj'
 *     C = L L', y = L^-1 r;  d2_prefix[hyp_ptr[h] + j] = sum of y_t^2 over t < 3 (j + 1)
 * Entry j is the joint distance of the hypothesis's first j + 1 candidates (compare with a chi^2 quantile of 3 (j + 1) degrees of freedom:
 * 16.27, 22.46, 27.88, 32.91 at 0.999 for 3, 6, 9, 12), the last entry the whole hypothesis's, the difference of consecutive entries
 * candidate j's distance conditioned on its predecessors: one call evaluates a whole branch of a branch-and-bound search, many hypotheses
 * one level of it.  Candidates may share nodes or repeat a pair, as (a, b) or as (b, a), also within one hypothesis.  Nodes, then unordered
 * node pairs, are deduplicated across ALL hypotheses of the call: a pair is solved once per call.  C, when not NULL, receives every
 * hypothesis's matrix, row-major and exactly symmetric, packed one after another (hypothesis h starts at the sum of 9 m_g^2 over g < h).
 * Two calls give the same bits; a hypothesis cut to its first j candidates and sent as a hypothesis of the same call reproduces prefix j
 * bit for bit; a one-candidate hypothesis agrees with aprilsam_amd_gate_xyt to rounding.
 * Returns 0, or the number of hypotheses in which a pivot of C was not positive (their d2_prefix entries are NaN from that candidate on;
 * W^-1 being positive definite this does not happen in exact arithmetic), or the codes of aprilsam_amd_gate_xyt: -1 no retained factor or
 * a resident run in progress; -12 sharded param, asymmetric W in the factorised graph, a candidate W that is not symmetric positive
 * definite; -13 a null argument, n_hyp < 0, a hyp_ptr that does not start at 0 or decreases, a hypothesis with 0 or more than
 * APRILSAM_AMD_JOINT_MAX candidates, a == b, a non-finite z or W, a node id out of range of the factorised system or of graph; -14 no HIP
 * device; -11 a buffer that does not fit under option mem_cap_mb.  What needs neither graph nor device (everything but the node ids) is
 * judged before a device is asked for.  n_hyp == 0 returns 0.  A refusal writes nothing and leaves plan, factor and Sigma in place. */
#define APRILSAM_AMD_JOINT_MAX 16      /* candidates per hypothesis */
int aprilsam_amd_marginals_set(april_graph_t *graph, april_graph_cholesky_param_t *param, int k, const int *nodes, double *cov);
int aprilsam_amd_gate_xyt_joint(april_graph_t *graph, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b,
                                const double *z, const double *W, double *d2_prefix, double *C);
/* debug: the largest path-solve work buffer this param has used, in bytes (-1: no context) */
long long aprilsam_amd_debug_path_solve_bytes(const april_graph_cholesky_param_t *param);

/* ---- information measures: log-determinants, set entropies, information gain ---------------------------------------
 * Three consumers of the retained factor.  All values are NATURAL logarithms (nats).  Common to the three: -1 no retained factor or a
 * resident run in progress (also after aprilsam_amd_optimize_lm / _gnc / aprilsam_amd_initialize_chordal, which drop the factor); -12
 * sharded param or asymmetric W in the factorised graph; -14 no HIP device; -11 a buffer that does not fit under option mem_cap_mb; -13 a
 * null argument.  A refusal writes nothing, sets aprilsam_amd_last_error and leaves plan, factor and Sigma in place; no selected inversion
 * runs and no Sigma pool is allocated.  Two calls give the same bits.
 *
 * aprilsam_amd_logdet: *logdet = ln det A of the system aprilsam_amd_solve documents, A = sum J^T W J + diag(lambda) = P' L L' P of the last
 * successful solver call on `param` (whichever way the step went: batch, tail fronts, low-rank updates, re-plan, batch fall-back; robust,
 * max-mixture, polar and Gaussian factors as they were factorised), computed as 2 sum ln L_jj over the factor's diagonal on the GPU.  A
 * fixed node's diagonal block of A is exactly the identity and contributes exactly 0: the result is the log-determinant of the REDUCED
 * system of the free nodes.  -ln det A is ln det of the whole joint covariance; the Laplace evidence of the linearised problem is
 * -chi2 / 2 - ln det A / 2 up to a constant.  The sum's order depends on the factor's structure alone: options that only move offsets or
 * reorder work lists give the same bits.  -15 if a diagonal entry is not positive and finite (an admitted factor has none).
 *
 * aprilsam_amd_logdet_sets: n_sets node sets, set_ptr (n_sets + 1 entries, set_ptr[0] == 0, CSR) indexing nodes; each set holds 1 ..
 * APRILSAM_AMD_SET_MAX DISTINCT nodes.  logdet_prefix[set_ptr[h] + j] = ln det Sigma of the joint marginal covariance of the set's first
 * j + 1 nodes -- the Sigma of aprilsam_amd_marginals_set -- by a Cholesky factorisation in LDS behind the path solves.  The last entry is
 * the whole set's value, the difference of consecutive entries the log-determinant of node j conditional on its predecessors.  With k
 * nodes in a set A (3 unknowns each):
 *     differential entropy   h(A)    = (3 k ln(2 pi e) + ln det Sigma_A) / 2
 *     mutual information     I(A; B) = (ln det Sigma_A + ln det Sigma_B - ln det Sigma_{A u B}) / 2
 * Nodes, then unordered pairs, are deduplicated across ALL sets of the call and solved once.  A set cut to its first j nodes, in this or
 * another call, reproduces prefix j bit for bit.  Returns 0, or the number of sets in which a pivot was not positive: their entries are
 * NaN from that node on.  A set that holds a fixed node is such a set (its rows of Sigma are exact zeros).  -13 also for n_sets < 0, a
 * set_ptr that does not start at 0 or decreases, an empty set or one of more than APRILSAM_AMD_SET_MAX nodes, a node repeated within a set
 * (all judged before a device is asked for), a node id out of range of the factorised system or of graph.  n_sets == 0 returns 0.
 *
 * aprilsam_amd_info_gain_xyt: the expected information gain of ADDING candidate xyt measurements between a[i] and b[i] with information
 * W[9i..]; the hypotheses have aprilsam_amd_gate_xyt_joint's shape (1 .. APRILSAM_AMD_JOINT_MAX candidates each, CSR hyp_ptr; candidates may
 * share nodes or repeat a pair).  gain_prefix[hyp_ptr[h] + j] = ln det (I + blockdiag(W_i) H Sigma H') / 2 over the hypothesis's first j + 1
 * candidates = (ln det C_prefix + sum_{i <= j} ln det W_i) / 2 with C = H Sigma_set H' + blockdiag(W_i^-1) exactly as _gate_xyt_joint
 * builds it: the Jacobians at the nodes' CURRENT states, Sigma at the l_points of the last solver call.  No z is taken: the Jacobians of an
 * xyt factor do not depend on the measurement, so the gain is known before the measurement exists.  Where states and l_points coincide,
 * 2 gain = ln det (A + H' W H) - ln det A: what aprilsam_amd_logdet would grow by if the factors were really added.  Every prefix is >= 0
 * and the prefixes do not decrease, up to rounding.  Argument rules, refusals and the return value (the number of hypotheses with a pivot
 * that was not positive, NaN from that candidate on) are _gate_xyt_joint's, without z: -12 also a W that is not symmetric positive
 * definite; -13 also a == b, a non-finite W, a bad hyp_ptr, a node id out of range.  n_hyp == 0 returns 0. */
#define APRILSAM_AMD_SET_MAX 16        /* nodes per set */
int aprilsam_amd_logdet(april_graph_t *graph, april_graph_cholesky_param_t *param, double *logdet);
int aprilsam_amd_logdet_sets(april_graph_t *graph, april_graph_cholesky_param_t *param, int n_sets, const int *set_ptr, const int *nodes,
                             double *logdet_prefix);
int aprilsam_amd_info_gain_xyt(april_graph_t *graph, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b,
                               const double *W, double *gain_prefix);

/* ---- solves with the retained factor -----------------------------------------------------------------------
 * The system is the one aprilsam_amd_marginals describes: A = sum J^T W J + diag(lambda) of the last successful solver call on `param`
 * (lambda where that step put it, everything at the l_points, robust and max factors as they were factorised).  Write A = P' L L' P with
 * P the permutation from node order to elimination order (a pose keeps its three consecutive rows).  aprilsam_amd_solve computes, for
 * nrhs right-hand sides,
 *     APRILSAM_AMD_SOLVE_FULL      X = A^-1 B
 *     APRILSAM_AMD_SOLVE_FORWARD   X = P' L^-1 P B        (X'X = B' Sigma B: whitening, Mahalanobis norms)
 *     APRILSAM_AMD_SOLVE_BACKWARD  X = P' L^-T P B        (E[X X'] = Sigma for white noise B: posterior samples)
 * B and X hold nrhs vectors of 3 N doubles each (vector r at offset r 3 N, node i's unknowns at 3 i .. 3 i + 2 in the order of delta_X; N
 * = the number of factorised nodes).  X == B is allowed, any other overlap is undefined.  FULL equals BACKWARD applied to FORWARD bit
 * for bit; the caller never needs the permutation.  Non-finite values in B propagate; a zero column gives a column that compares equal
 * to 0.0.  The columns are processed in chunks (multiples of 16) so that the work buffer -- (sum over the fronts of rows) x columns
 * doubles -- stays under 1 GB or option mem_cap_mb, one tile of 16 columns at the least; option solve_chunk_cols forces the width.  The
 * results do not depend on the chunking, and two calls give the same bits.
 * Returns 0, or the codes of aprilsam_amd_marginals: -1 no retained factor or a resident run in progress (also after
 * aprilsam_amd_optimize_lm / _gnc / aprilsam_amd_initialize_chordal, which drop the factor); -12 sharded param or asymmetric W in the
 * factorised graph; -13 a null argument, mode outside 0..2, nrhs < 1, anchor or a node out of range of the factorised system (for
 * aprilsam_amd_relative_covariances also of graph); -14 no HIP device; -11 the work buffer does not fit under option mem_cap_mb.  A
 * refused or failed call writes nothing to X / cov (the chunks of a call are kept back until the last one has succeeded), sets aprilsam_amd_last_error and leaves plan, factor and Sigma in place. */
enum { APRILSAM_AMD_SOLVE_FULL = 0, APRILSAM_AMD_SOLVE_FORWARD = 1, APRILSAM_AMD_SOLVE_BACKWARD = 2 };
int aprilsam_amd_solve(april_graph_t *graph, april_graph_cholesky_param_t *param, int mode, int nrhs, const double *B, double *X);
/* Sigma_{node, anchor} for the n listed nodes (nodes == NULL: all N nodes, n ignored): 9 doubles per node, row-major, the node's unknowns
 * as rows.  One FULL solve of the anchor's three unit columns over the whole tree, then an extraction. */
int aprilsam_amd_marginals_cross(april_graph_t *graph, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov);
/* The covariance of the predicted xyt measurement x_anchor^-1 o x_i in the anchor's frame for the n listed nodes i (NULL: all), 9 doubles
 * each, row-major:  [J_a J_i] [[S_aa S_ai]; [S_ia S_ii]] [J_a J_i]'  with the Jacobians an xyt factor computes at the nodes' CURRENT
 * states, exactly as aprilsam_amd_gate_xyt takes them: the result equals gate_xyt's S - W^-1 for the pair (anchor, i).  S_ai comes from
 * the column solve, S_aa and S_ii from the selected inversion's Sigma pool: the first call after a solver call runs the inversion as
 * aprilsam_amd_marginals does.  i == anchor gives exact zeros. */
int aprilsam_amd_relative_covariances(april_graph_t *graph, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov);
/* N of the calls above: the nodes of the system the retained factor of `param` was made for, or -1 when there is none (no device needed).
 * It takes no graph, so it cannot see a node fixed or freed since the factorisation (fixed nodes, below): it answers N until a consumer
 * that takes the graph has seen the toggle and dropped the factor, -1 from then on. */
int aprilsam_amd_factorised_nodes(const april_graph_cholesky_param_t *param);
/* debug: the largest whole-tree work buffer this param has used, in bytes (-1: no context) */
long long aprilsam_amd_debug_solve_bytes(const april_graph_cholesky_param_t *param);

/* ---- Levenberg-Marquardt optimisation -------------------------------------------------------------------
 * The reference has no counterpart: april_graph_cholesky is one Gauss-Newton step with the fixed damping param->tikhanov, and the
 * drop-in entry points keep exactly that.  aprilsam_amd_optimize_lm runs a whole damped optimisation on the GPU, every iteration one
 * captured graph; the accept / reject decision is made on the device and the host only polls a small status block.
 *   Objective  F(x) = sum_f r_f' W_f r_f over all factors, NO 0.5 factor: the cost the normal equations (sum J'WJ + D) h = sum J'W r
 *              minimise (april_graph_chi2 halves xyt terms and would not match the model).  A max factor contributes
 *              min_k (r_k' W_k r_k + c_k), c_k = -2 log w_k - ln det W_k: the score its selection minimises.
 *   Damping    D = lambda on every pose, written into the device's damping array by the device.  param->tikhanov is the reference's
 *              fixed Tikhonov term of the plain step; the LM run ignores it (it would bound the damping from below).
 *   Iteration  at the current point x (state = l_point = x, so xytpos priors linearise at the same point):
 *              1. select the max-factor components at x;  2. linearise, assemble, factor, back-substitute (the existing kernels); the
 *              update goes to a trial buffer, x_t = x (+) h, theta wrapped;  3. F(x_t);  4. the model decrease
 *              pred = sum_f [r_f' W_f r_f - (r_f - d_f)' W_f (r_f - d_f)] = sum_f d_f' W_f (2 r_f - d_f), d_f = J_a h_a + J_b h_b, at x
 *              with the selected slot's z and W (it equals h'B + lambda |h|^2);  5. rho = (F(x) - F(x_t)) / pred.
 *   Rejection  a pivot that was not positive, a NaN in h or a non-finite F(x_t) rejects the step (rejected_not_spd counts the first).
 *   Decision   (Nielsen) rho > eta: x <- x_t, lambda <- lambda * max(1/3, 1 - (2 rho - 1)^3), nu <- 2; otherwise lambda <- lambda * nu,
 *              nu <- 2 nu.  pred <= 0 on a step that was not rejected: converged (status CONVERGED_F).  After an accepted step the
 *              ftol test, then the xtol test; lambda > lambda_max: STALLED; max_iters iterations: MAX_ITERS.
 *   Determinism  once a stop condition holds, every later iteration of the same chunk of check_every iterations is a no-op (a device
 *              latch): results and trace are bitwise the same for every check_every, and two runs give identical bits.
 * What the call leaves: state = l_point = x*, the last accepted iterate (x0 if none); delta_X = the last accepted h (untouched if none);
 * param->tikhanov untouched; the param's plan kept; the retained factor DROPPED (it was made at another point with another lambda):
 * aprilsam_amd_marginals* / aprilsam_amd_gate_xyt return -1 and the next april_graph_cholesky_inc behaves as on a fresh param.  For
 * covariances at the optimum call april_graph_cholesky once, then aprilsam_amd_marginals.
 * Returns 0 (reason in report->status), or: -1 empty graph; -4 the graph holds host-evaluated (foreign) factors; -12 sharded param, or
 * a factor with an asymmetric information matrix; -13 bad options or a null argument; -14 no HIP device.  On a refusal nothing is
 * written and the graph is untouched; aprilsam_amd_last_error says why.  A failure during the run fails the call as on every solver
 * entry point (see the error codes above): -9 when a multi-level launch of an iteration gave up waiting for a dependency flag (never
 * taken for a rejected step), -10 / -11 for HIP errors / memory; the graph is untouched and the param's plan and captured graphs are
 * dropped. */
typedef struct {
    int    max_iters;     /* >= 1, default 50: LM iterations (accepted + rejected) */
    int    check_every;   /* >= 1, default 1: the host reads the status after this many iterations; results never depend on it */
    double lambda0;       /* > 0, default 1e-4: initial damping */
    double lambda_max;    /* default 1e16: damping above this ends the run, status STALLED */
    double eta;           /* default 0, in [0, 1): a step is accepted when rho > eta */
    double ftol;          /* default 1e-10: an accepted step with F - F_new <= ftol * |F| ends the run, CONVERGED_F */
    double xtol;          /* default 1e-10: an accepted step with ||h||_2 <= xtol * (||x||_2 + xtol) ends the run, CONVERGED_X */
} aprilsam_amd_lm_opts_t;
void aprilsam_amd_lm_opts_init(aprilsam_amd_lm_opts_t *opts);

enum { APRILSAM_AMD_LM_CONVERGED_F = 1, APRILSAM_AMD_LM_CONVERGED_X = 2, APRILSAM_AMD_LM_STALLED = 3, APRILSAM_AMD_LM_MAX_ITERS = 4 };
typedef struct {
    int    status, iterations, accepted, rejected_not_spd;
    double F_initial, F_final;     /* the LM objective above */
    double chi2_final;             /* april_graph_chi2 of the returned states */
    double lambda_final;
} aprilsam_amd_lm_report_t;

/* trace: NULL, or 4 * opts->max_iters doubles, one row per iteration: F at the trial point, rho, the lambda used, accepted (0/1) */
int aprilsam_amd_optimize_lm(april_graph_t *graph, april_graph_cholesky_param_t *param, const aprilsam_amd_lm_opts_t *opts,
                             aprilsam_amd_lm_report_t *report, double *trace);

/* ---- chordal initialisation (Carlone et al., ICRA 2015) -----------------------------------------------------
 * Every optimiser above starts from the states the caller supplies; from a poor start LM does not reach the optimum.
 * aprilsam_amd_initialize_chordal computes a start from the factors alone -- it reads no state -- as two linear least-squares problems on
 * the graph's own sparsity pattern, each solved by the plan, assembly, factorisation and back substitution of a batch step, damping 0.
 *   Stage 1    headings.  Unknown u_i = (c_i, s_i) per pose.  An xyt factor (a, b, z, W) with w = W[2][2] > 0 contributes
 *              w |R(z_theta) u_a - u_b|^2, an xytpos prior with w > 0 contributes w |u_a - (cos z_theta, sin z_theta)|^2.  Then
 *              theta_i = atan2(s_i, c_i); a pose with c^2 + s^2 == 0 or a non-finite value keeps its incoming heading (n_degenerate).
 *   Stage 2    positions, headings held fixed.  Unknown t_i per pose, Wxy = W[0:2, 0:2].  An xyt factor with W[0][0] > 0 and
 *              det Wxy > 0 contributes |R(theta_a)' (t_b - t_a) - z_xy|^2_Wxy, a prior under the same condition |t_a - z_xy|^2_Wxy.
 *   A factor that fails a stage's condition contributes nothing to that stage (an xy-only prior enters stage 2 only); the xy-theta cross
 *   terms of W are ignored.  A robust loss is ignored (the plain W is used); a max factor enters as the component with the largest log
 *   weight, lowest index on a tie.
 * What the call leaves: state = l_point = the initial guess; delta_X and param->tikhanov untouched; the param's plan kept; the retained
 * factor DROPPED as after aprilsam_amd_optimize_lm (marginals and gating return -1 until the next april_graph_cholesky).  Two calls give
 * identical bits, and the result does not depend on the incoming states (degenerate poses and stages = 1 apart).
 * Typical use: aprilsam_amd_initialize_chordal, then aprilsam_amd_optimize_lm.
 * Returns 0, or: -1 empty graph; -4 host-evaluated (foreign) factors; -12 sharded param, or an information matrix that is not symmetric;
 * -13 a null argument or bad stages; -14 no HIP device; -2 the system of a stage is not positive definite (a graph without a heading
 * prior, a part of the graph that no prior reaches): report->not_spd_stage says which.  On a refusal the graph is untouched and nothing
 * is written -- except the report on -2; aprilsam_amd_last_error says why.  A failure during the run (-9 / -10 / -11) behaves as on
 * every solver entry point. */
typedef struct {
    int    stages;        /* 3 = both (default), 1 = headings only: positions keep their incoming values */
} aprilsam_amd_chordal_opts_t;
void aprilsam_amd_chordal_opts_init(aprilsam_amd_chordal_opts_t *opts);
typedef struct {
    int    status;                 /* 0 ok (-2 on that refusal) */
    int    n_degenerate;           /* poses that kept their incoming heading */
    int    not_spd_stage;          /* 0, 1 or 2 */
    double min_norm;               /* min_i |u_i| (0 when a pose is degenerate) */
    double F_initial, F_final;     /* LM's objective at the incoming / returned states */
} aprilsam_amd_chordal_report_t;
/* rot_out: NULL or 2*N doubles, (c_i, s_i) of stage 1 in node order, before normalisation */
int aprilsam_amd_initialize_chordal(april_graph_t *graph, april_graph_cholesky_param_t *param, const aprilsam_amd_chordal_opts_t *opts,
                                    aprilsam_amd_chordal_report_t *report, double *rot_out);
/* debug: the same call; raw: 6*N doubles, the solution of stage 1 then of stage 2 (3 per pose, node order) with the padded third unknown */
int aprilsam_amd_debug_chordal_raw(april_graph_t *graph, april_graph_cholesky_param_t *param, const aprilsam_amd_chordal_opts_t *opts,
                                   aprilsam_amd_chordal_report_t *report, double *raw);

/* ---- max-mixture factors (Olson & Agarwal, RSS 2012) ---------------------------------------------------
 * A max factor on the ordered pair (a, b) holds K = 1..8 components, each an xyt factor made by april_graph_factor_xyt_create on
 * the same (a, b) with a symmetric W of det W > 0, and a log weight per component.  At a point p component i scores
 *     s_i = r_i(p)^T W_i r_i(p) - 2 logw_i - ln det W_i           (r_i: the xyt residual, mod2pi on theta)
 * and the selected component is  best = 0; for i in 1..K-1: if (s_i < s_best) best = i  (ties and NaN: the lower index).
 * Wherever the solver linearises the factor it selects at the factor's linearisation point (l_point of a and b), on the GPU, and
 * linearises the selected component exactly as an xyt factor; an incremental step selects a new factor when it first linearises
 * it.  april_graph_chi2 counts 0.5 r_s^T W_s r_s with s selected at the states.  With K = 1 and logw = 0 the factor is its single
 * component, bit for bit.  The layout is the reference's u.max { factors, logw, nfactors }; eval / state_eval return the selected
 * component's evaluation at l_point / state, copy is deep, destroy frees the components.
 * A factor is native only if type == APRILSAM_AMD_FACTOR_MAX_TYPE AND its eval is this library's: a foreign factor that uses tag 3
 * keeps the host-evaluated path.  Sharded runs refuse max factors (-12); .graph files cannot hold them (save returns an error). */
#define APRILSAM_AMD_FACTOR_MAX_TYPE 3
/* takes ownership of components[0..n); copies logw; NULL (+ aprilsam_amd_last_error, -12) on a bad argument, owning nothing then */
april_graph_factor_t *aprilsam_amd_factor_max_create(april_graph_factor_t **components, const double *logw, int n);
/* for each listed graph factor: index of the component its most recent linearisation used, -1 for a non-max factor or one not yet
 * linearised; returns 0 or a negative error code (-13 for an index out of range or a bad argument) */
int aprilsam_amd_max_selected(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *factors, int *out);

/* ---- robust losses on xyt / xytpos factors (iteratively reweighted least squares) ----------------------------
 * A library-made xyt factor (april_graph_factor_xyt_create) or xytpos factor (april_graph_factor_xytpos_create) may carry a loss kind and
 * a scale c (finite, > 0), a threshold on the Mahalanobis distance sqrt(s).  Its W must be symmetric (mirror entries bitwise equal) with
 * all three leading minors > 0.  With r the plain factor's residual (theta wrapped) and s = r' W r:
 *     HUBER   rho = s if s <= c^2, else 2 c sqrt(s) - c^2          w = 1 if s <= c^2, else c / sqrt(s)
 *     CAUCHY  rho = c^2 log1p(s / c^2)                              w = 1 / (1 + s / c^2)
 *     DCS     rho = s if s <= c^2, else c^2 (3 s - c^2) / (s + c^2)  w = 1 if s <= c^2, else 4 c^4 / (s + c^2)^2
 * (DCS: dynamic covariance scaling, Agarwal et al., ICRA 2013, Phi = c^2.)  A NaN s gives a NaN weight: the call fails as for a plain
 * factor that went non-finite.  Wherever the solver linearises the factor -- batch, resident and LM steps on the GPU, every fall-back
 * of an incremental run -- it linearises the plain factor with W_eff = w(s) * W (one multiply per entry), s taken at the factor's
 * linearisation point (xyt: the l_points; xytpos: the node's state, as the plain prior).  An incremental fast step weights a NEW
 * robust factor on the host when it first linearises it; older factors keep their weight until a fall-back re-linearises everything.
 * april_graph_chi2 and aprilsam_amd_resident_chi2 count 0.5 rho(s) for an xyt factor and rho(s) for an xytpos factor; the LM objective
 * counts rho(s), and its model decrease is that of the weighted system solved.  Marginals, joint covariances and gating describe the
 * system that was factorised: the weighted one.  eval / state_eval return the plain r and J with W = w(s) W and chi2 = rho(s).
 * Sharded runs refuse robust factors (-12); .graph files cannot hold them (save returns 0 and writes nothing); max factors refuse
 * components that carry a loss (-12). */
enum { APRILSAM_AMD_ROBUST_NONE = 0, APRILSAM_AMD_ROBUST_HUBER = 1, APRILSAM_AMD_ROBUST_CAUCHY = 2, APRILSAM_AMD_ROBUST_DCS = 3 };
/* kind NONE clears the loss; 0, -12 (not a library xyt / xytpos factor, a max factor, W not symmetric positive definite), -13 (NULL, kind
 * out of range, c not finite or <= 0); sets aprilsam_amd_last_error on failure, factor unchanged then */
int aprilsam_amd_factor_set_robust(april_graph_factor_t *factor, int kind, double c);
int aprilsam_amd_factor_get_robust(const april_graph_factor_t *factor, int *kind, double *c);   /* NONE / 0 for any other factor */
/* for each listed graph factor: the weight its most recent linearisation used; -1 for a non-robust factor or one not yet linearised.
 * Returns 0 or -13 (an index out of range or a bad argument) */
int aprilsam_amd_robust_weights(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *factors, double *w);

/* ---- range, bearing and range-bearing factors ------------------------------------------------------------------
 * Measurements whose noise is Gaussian in POLAR coordinates: UWB or sonar ranges, a camera's bearing to a tag, the range-bearing
 * observation of a landmark.  Node a observes node b.  With q the position of b in a's frame (what an xyt factor predicts as its first
 * two components), rho = |q| and beta = atan2(q1, q0):
 *     RANGE          z = {rho}          W = {w}
 *     BEARING        z = {beta}         W = {w}
 *     RANGE_BEARING  z = {rho, beta}    W 2 x 2 row-major
 * The residual is z - h(q), its bearing component wrapped with mod2pi; b's heading never enters.  W must be finite, symmetric (mirror
 * entries bitwise equal) and positive definite, z finite, a != b.
 * The object is a valid reference factor: nnodes = 2, length = m (1 or 2), u.common.z holds m doubles, u.common.W is an m x m matd;
 * eval / state_eval return the true m-row r, J, W and chi2 = r' W r at l_point / state; copy is deep.  april_graph_chi2 and
 * aprilsam_amd_resident_chi2 count the full r' W r (the reference's rule for every type but xyt, april_graph.c:86-94), at the states;
 * the LM objective counts the same.
 * Wherever the solver linearises the factor -- batch, resident, LM and GNC steps on the GPU, every fall-back of an incremental run -- a
 * kernel writes the xyt slot  W_eff = [[G' W G, 0], [0, 0]],  z_eff = (q + G' (G G')^-1 r, zh2)  with G = dh/dq at the linearisation
 * point, and the factor is linearised as that xyt factor: its contribution to the normal equations is exactly J' W J and J' W r of the
 * m-row factor.  An incremental fast step writes a NEW factor's slot on the host when it first linearises it.  If rho^2 == 0 at the
 * linearisation point the factor is silent for that step (W_eff = 0); there is no threshold, a tiny non-zero rho keeps its 1 / rho
 * Jacobian.  A non-finite input fails the call as a plain factor that went non-finite does.
 * A LANDMARK is an ordinary xyt node, and nothing observes its heading: give it param->tikhanov > 0 (the default), LM's damping, or an
 * xytpos prior with W = diag(0, 0, w) -- otherwise the system is singular in that heading.  april_graph_cholesky_inc puts no tikhanov term
 * on the nodes it adds (aprilsam.c:508-542): a landmark that arrives in an incremental step needs the prior.
 * A factor is native only if type == APRILSAM_AMD_FACTOR_POLAR_TYPE AND its eval is this library's: a foreign factor that uses tag 4 keeps
 * the host-evaluated path.  Not supported, refused with -12: a robust loss on a polar factor, a polar factor as a max component or as a
 * GNC candidate, aprilsam_amd_initialize_chordal on a graph that holds one (it carries no relative heading), sharded params; .graph files
 * cannot hold them (save returns 0 and writes nothing).  Debug option "polar_on_host" = 1 packs polar factors as host-evaluated foreign
 * factors through their own eval() (the A/B oracle of the tests; april_graph_chi2 then takes their term from state_eval). */
enum { APRILSAM_AMD_POLAR_RANGE = 1, APRILSAM_AMD_POLAR_BEARING = 2, APRILSAM_AMD_POLAR_RANGE_BEARING = 3 };
#define APRILSAM_AMD_FACTOR_POLAR_TYPE 4
/* copies z and W; NULL (+ aprilsam_amd_last_error: -12 for W, -13 otherwise) on a bad argument, owning nothing then */
april_graph_factor_t *aprilsam_amd_factor_polar_create(int kind, int a, int b, const double *z, const double *W);
int aprilsam_amd_factor_get_polar(const april_graph_factor_t *factor, int *kind);      /* 0 for any other factor */
/* debug, host only, no device: the slot (z_eff: 3, W_eff: 9 row-major) of a polar factor at poses pa, pb -- the formulas host and kernels
 * share.  0, or -13 on a bad argument */
int aprilsam_amd_debug_polar_slot(int kind, const double *pa, const double *pb, const double *z, const double *W, double *z_eff3, double *W_eff9);

/* ---- dense Gaussian factor on k nodes, information form -----------------------------------------------------------
 * What is left on the Markov blanket of poses that were eliminated from a graph: a dense Gaussian, usually rank-deficient (a relative
 * constraint among the blanket nodes, no absolute information).  With delta = x (-) xbar the per-node difference (3 k entries, the heading
 * components wrapped with mod2pi), the factor contributes
 *     H = Lambda          g = eta - Lambda delta                     to the normal equations A dx = g
 * with delta taken at the nodes' l_points when linearising, and the term
 *     c0 - 2 eta' delta + delta' Lambda delta                        to chi^2 and to the LM objective
 * with delta taken at the states.  c0 = d'd, where R'R = Lambda and R'd = eta (below): the smallest constant that keeps the term >= 0
 * (the kernel's rounding is cut off at 0).
 * Lambda (3 k x 3 k, row-major) must be finite, symmetric (mirror entries bitwise equal) and positive SEMI-definite -- singular is the
 * normal case; xbar and eta finite; the node ids distinct; 1 <= k <= APRILSAM_AMD_GAUSSIAN_MAX_NODES.
 * The object is a valid reference factor: nnodes = k, u.common.z holds xbar (3 k) followed by eta (3 k), u.common.W is Lambda as a
 * 3 k x 3 k matd, copy is deep.  At creation a diagonally pivoted Cholesky of Lambda (LAPACK dpstrf's default stop: the largest
 * remaining diagonal <= 3 k eps max diag Lambda; a remaining diagonal below minus that bound refuses the matrix) gives R (rank x 3 k)
 * with R'R = Lambda and, by a triangular solve in pivot order, d with R'd = eta in the least-squares sense.  length = rank;
 * eval / state_eval return length = rank, J = R split per node, W = I, r = d - R delta and chi2 = r'r at l_point / state.  z and W may
 * be edited in place: every evaluation and every solver call compares them with what R was made from and factorises again on a change
 * (a W that is no longer admissible fails that solver call with -12).
 * The solver keeps the factor as the clique of its k (k - 1) / 2 node pairs (one entry for k <= 2), so ordering, symbolic analysis and
 * factorisation do not know it; a kernel (one wave per factor) writes Lambda's blocks and g into the pairs' contribution slots after the
 * linearisation kernel and before the fixed-node mask.
 * Open: april_graph_cholesky, aprilsam_amd_batch_resident and the resident loop, LM, GNC (as a non-candidate), aprilsam_amd_debug_stage,
 * aprilsam_amd_solve, marginals, joint covariances, both gating calls, fixed nodes, april_graph_chi2 / aprilsam_amd_resident_chi2.
 * Refused with -12, nothing written: april_graph_cholesky_inc and april_graph_cholesky_inc_solver on a graph that holds such a factor,
 * aprilsam_amd_initialize_chordal, sharded params, a robust loss on it, its use as a max component or GNC candidate, k > 11.
 * aprilsam_amd_factor_audit counts it among the factors it cannot audit (four NaN).  .graph files cannot hold it (save returns 0 and
 * writes nothing).  A factor is native only if type == APRILSAM_AMD_FACTOR_GAUSSIAN_TYPE AND its eval is this library's.  Debug option
 * "gaussian_on_host" = 1 packs it as a host-evaluated clique through its own eval() (the A/B oracle of the tests; april_graph_chi2 then
 * takes its term from state_eval). */
#define APRILSAM_AMD_FACTOR_GAUSSIAN_TYPE 5
#define APRILSAM_AMD_GAUSSIAN_MAX_NODES 11      /* the clique limit of factors with more than two nodes: 55 pairs */
/* copies everything; NULL (+ aprilsam_amd_last_error: -12 for Lambda or k > 11, -13 otherwise) on a bad argument, owning nothing then */
april_graph_factor_t *aprilsam_amd_factor_gaussian_create(int k, const int *nodes, const double *xbar /*3k*/, const double *eta /*3k*/,
                                                          const double *Lambda /*3k x 3k row-major*/);
int aprilsam_amd_factor_get_gaussian(const april_graph_factor_t *factor, int *k);   /* 0 for any other factor */

/* ---- marginalising poses out of a graph ----------------------------------------------------------------------------
 * aprilsam_amd_marginal_prior: the dense Gaussian that eliminating the nodes M = remove[0, m) (distinct, in range) leaves on their
 * Markov blanket.  F_M = the packed factors with an endpoint in M; B = their other endpoints, ascending, returned in keep.  With H and g
 * summed from the linearisation of F_M ONLY, as the param's last factorisation saw it (robust weights, the selected mixture component,
 * polar slots and another Gaussian factor's blocks count as they stand; no tikhanov term, no LM damping), ordered M first:
 *     Lambda = H_BB - H_BM H_MM^-1 H_MB        eta = g_B - H_BM H_MM^-1 g_M        xbar = the linearisation point of the nodes in B
 * computed on the GPU by one workgroup from the contribution slots the factorisation left on the device (two calls give the same bits).
 * THE PRIOR IS EXACT AT THE LINEARISATION POINT OF THE LAST SOLVE: a caller who wants the exact marginal marginalises after convergence,
 * or with the states reset to the l_points.
 * Available exactly when aprilsam_amd_factor_audit is, with its codes: -1 (no retained factor of this graph, or the graph's device copy no
 * longer holds this param's linearisation), -12 (sharded param, asymmetric W, the retained factor is an incremental step's extended
 * structure), -13 (bad argument, an id out of range or listed twice), -14.  Also -12, nothing written: |M| + |B| >
 * APRILSAM_AMD_MARGINAL_MAX_NODES; |B| > cap; a fixed node in M or B (its slots are masked); a graph factor of more than two nodes -- a
 * host-evaluated clique or a Gaussian factor with k >= 3 -- touching M (a host-evaluated factor of one or two nodes is fine).  A pivot of
 * H_MM that is not positive or not finite: -2 through aprilsam_amd_last_error, nothing written; the param keeps its factorisation
 * (the removed block is not what it factorised).  m == 0: returns 0 with *n_keep = 0.  B empty (a component removed whole): H_MM is still
 * checked; returns 0 with *n_keep = 0 and nothing else written.
 * Outputs: *n_keep = |B|, keep[|B|], xbar[3 |B|], eta[3 |B|], Lambda[(3 |B|)^2] row-major, written densely, symmetric bit for bit. */
#define APRILSAM_AMD_MARGINAL_MAX_NODES 40      /* |M| + |B|: the system is 120 x 121 doubles = 116 KB of one workgroup's LDS */
int aprilsam_amd_marginal_prior(april_graph_t *graph, april_graph_cholesky_param_t *param, int m, const int *remove, int cap, int *n_keep,
                                int *keep /*cap*/, double *xbar /*3 cap*/, double *eta /*3 cap*/, double *Lambda /*(3 n_keep)^2*/);
/* Host only, no device: destroys the nodes remove[0, m) and every factor with a node among them (a max-mixture factor is judged by its own
 * nodes), closes the gaps in both arrays keeping their order, renumbers nodes[] of every remaining factor AND of every max component, and
 * writes new_index[old] = new, or -1 for a removed node (old N entries; may be NULL).  The graph's device copy is dropped.  Everything is
 * validated first: -13 (an id out of range or listed twice, a factor that names a node outside the graph) leaves the graph untouched.  0 on
 * success. */
int aprilsam_amd_graph_remove_nodes(april_graph_t *graph, int m, const int *remove, int *new_index /*old N entries or NULL*/);
/* aprilsam_amd_marginal_prior, then aprilsam_amd_factor_gaussian_create on B, then aprilsam_amd_graph_remove_nodes, then the factor appended
 * with renumbered ids.  All or nothing: every refusal above (and |B| > APRILSAM_AMD_GAUSSIAN_MAX_NODES: -12, the message names |B|)
 * returns before the graph is touched.  Returns the new factor's index; 0 with no factor when B is empty; or the code.  The param's plan and
 * retained factor are dropped: the next call plans the smaller graph. */
int aprilsam_amd_graph_marginalize(april_graph_t *graph, april_graph_cholesky_param_t *param, int m, const int *remove, int *new_index);

/* ---- gating and association of range / bearing observations against landmarks ------------------------------------
 * The step before aprilsam_amd_factor_polar_create: does a candidate measurement (kind, z, W as above; node a observes node b) agree
 * with what the solved graph predicts?  Per candidate, on the GPU right after the path solves of aprilsam_amd_marginals_joint_any:
 *     q, r    the position of b in a's frame and r = z - h(q), the bearing wrapped, at the nodes' CURRENT states (as aprilsam_amd_gate_xyt)
 *     J_p     G J_q: G = dh/dq (m x 2), J_q = rows 0 and 1 of the xyt factor's [J_a J_b] (2 x 6; b's heading column is zero)
 *     S  = J_p Sigma_ab J_p' + W^-1       Sigma_ab: aprilsam_amd_marginals_joint_any's block, at the l_points of the last solver call
 *     d2 = r' S^-1 r                      m = 1 (RANGE, BEARING) or 2 (RANGE_BEARING) degrees of freedom: chi^2 0.999 quantiles 10.83 / 13.82
 * A range-bearing candidate and its xyt twin (W_xyt = blockdiag(G' W G, w_theta), a zero heading residual) agree: S = G S_xyt[:2, :2] G'
 * exactly, so d2 is the d2 of the first two rows of aprilsam_amd_gate_xyt's S with the residual in polar coordinates; with the xyt
 * residual itself for the twin whose z is (q + G^-1 r, predicted heading) -- the same z in Cartesian form to first order in r.
 * Layout: z[2 i ..], W[4 i ..] (row-major 2 x 2), S[4 i ..] (row-major 2 x 2, or NULL).  A 1-row kind reads z[2 i] and W[4 i] only and
 * writes S[4 i], with 0 in the three entries behind it.  If rho^2 == 0 at the current states G does not exist: d2 and the m x m entries
 * of S are NaN for that candidate (no threshold, as for the factor).  Every distinct pair (a, b) is solved once, however many candidates
 * name it.  With fixed nodes (section 20) a fixed landmark is gated with the observer's covariance alone.
 *
 * aprilsam_amd_associate_polar: m observations made from node `observer` against the L nodes landmarks[0..L): the L pairs are solved once
 * (not m times), every (observation, landmark) entry is gated and reduced on the GPU.  Per observation i:
 *     best[i]        the index INTO landmarks of the smallest d2 if that d2 <= gate1 (1-row kind) / gate2 (2-row kind), else -1: a new
 *                    landmark.  Ties go to the lower index, so a landmark listed twice resolves to its first listing.
 *     d2_best[i], d2_second[i]   the two smallest d2 over all L whatever the gate says (NaN entries skipped); +inf where fewer than one /
 *                    two exist: the caller's ambiguity test
 *     d2[i L + l]    the whole matrix, or NULL
 * This is nearest-neighbour association: two observations may choose the same landmark.
 * Both return >= 0: the number of candidates / of (observation, landmark) entries that were unavailable because rho^2 == 0; or the codes
 * of aprilsam_amd_gate_xyt: -1 no retained factor; -12 sharded param, asymmetric W in the factorised graph, a W that is not symmetric
 * positive definite; -13 a null argument, a negative count, a kind outside the three, a == b or the observer among the
 * landmarks, a non-finite z or W entry that is read, a non-finite gate, a node id out of range of the factorised system or of graph;
 * -14 no HIP device.  What can be judged without the graph (null, counts, kinds, a == b, z, W, gates) is judged before a device is asked
 * for.  A refusal writes nothing and leaves plan, factor and Sigma alone.  n == 0, m == 0 or L == 0 return 0; with L == 0 every best is
 * -1 and d2_best, d2_second are +inf.  Two calls give the same bits, and the matrix equals aprilsam_amd_gate_polar on the expanded list
 * bit for bit. */
int aprilsam_amd_gate_polar(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, const int *kind,
                            const double *z, const double *W, double *d2, double *S);
int aprilsam_amd_associate_polar(april_graph_t *graph, april_graph_cholesky_param_t *param, int observer, int m, const int *kind, const double *z,
                                 const double *W, int L, const int *landmarks, double gate1, double gate2, double *d2, int *best,
                                 double *d2_best, double *d2_second);
/* debug, host only, no device: d2 and S (4 doubles, laid out as above) of one candidate at poses pa, pb with the 6 x 6 joint block cov36
 * (row-major, a's unknowns first) -- the function host and kernels share.  0; 1 when rho^2 == 0 (NaN written); -13 on a bad argument */
int aprilsam_amd_debug_polar_gate(int kind, const double *pa, const double *pb, const double *z, const double *W, const double *cov36,
                                  double *d2, double *S4);

/* ---- per-factor audit: leverage and leave-one-out distance ------------------------------------------------------
 * Which factors ALREADY in the graph does the rest of the graph contradict, and which can nothing check at all?  Answered on the GPU for
 * the linear system A the last successful solver call factorised, Sigma = A^-1 at that call's linearisation points lp, Delta the step it
 * solved (the nodes' delta_X).  Like the covariance calls, it describes the system that was factorised: every factor is taken in the
 * xyt form (a, b, z, W) its linearisation slot held -- a robust factor with W_eff = w W, a max-mixture with the component that was
 * selected, a range / bearing factor as its xyt slot (exact: r_eff' W_eff r_eff = r_p' W_p r_p at lp, W_eff of rank 1 or 2); b < 0 is an
 * xytpos prior.  Per listed factor f:
 *     J = [J_a J_b], r     the factor's Jacobians and residual (theta wrapped) at lp; J = I for a prior
 *     v = r - (J_a Delta_a + J_b Delta_b)      the linear model's post-fit residual
 *     P = J Sigma_ff J'    Sigma_ff: the 3 x 3 / 6 x 6 block of f's nodes (always on the pattern of L); rows and columns of a node that
 *                          was fixed are exact zeros
 *     M = I - P W
 * out[4 i ..] =
 *     chi2          v' W v         the factor's share of the linear system's cost
 *     leverage      tr(P W)        in [0, rank W]: degrees of freedom the factor spends; rank W - leverage is its redundancy number
 *     d2_loo        v' W M^-1 v    the Mahalanobis distance of f against the same linear system WITHOUT f (where W is regular:
 *                                  v' (W^-1 - P)^-1 v): compare with the chi^2 quantiles quoted at aprilsam_amd_gate_xyt.  NaN when det M <= 0
 *                                  or is not finite
 *     checkability  det M          in [0, 1]; 0: f is the only information on some direction (a bridge, a lone prior) and d2_loo means
 *                                  nothing, however small chi2 is
 * No threshold is applied: the caller reads checkability and decides.  A factor between two fixed nodes gives 0, 1 and d2_loo == chi2.
 * factors == NULL: all graph factors of the factorised system, in graph order (n ignored).
 * Returns >= 0: the number of listed factors that cannot be audited, four NaN each -- the factors evaluated on the host through eval()
 * (foreign types, more than two nodes): they have no slot and user code is not called back.  Or the codes of aprilsam_amd_marginals:
 * -1 no retained factor (also after aprilsam_amd_optimize_lm / _gnc / _initialize_chordal, during a resident run, or when the param's
 * last call was made with another graph, or the graph's device copy no longer holds THIS param's linearisation: lp, Delta and the slots
 * live with the graph, shared by every param that solves it, so another param's solver call on the graph -- a step, an LM or GNC run, a
 * failed call -- an april_graph_cholesky_inc_solver call, or a factor's z / W edited and then evaluated by april_graph_chi2 ends the
 * audit's availability until this param's next batch call; april_graph_chi2 alone does not); -12 sharded param, asymmetric W in the factorised graph, or the retained factor is the extended
 * structure of a fast april_graph_cholesky_inc step (its slots are no consistent picture of that system: a batch call makes the audit
 * available); -13 null argument, n < 0, a factor index outside the factors that call packed (factors added since), a node count that
 * differs from the factorised one, or a graph that holds fewer factors than the factorised system; -14 no HIP device; -11 the Sigma pool does not fit under mem_cap_mb.  A refused or failed call writes
 * nothing, sets aprilsam_amd_last_error and leaves plan, factor and Sigma in place; two calls give the same bits; a second call with no
 * solver call in between runs no selected inversion.  Available after april_graph_cholesky, aprilsam_amd_batch_resident,
 * aprilsam_amd_resident_end and an april_graph_cholesky_inc call that fell back to a batch step. */
int aprilsam_amd_factor_audit(april_graph_t *graph, april_graph_cholesky_param_t *param, int n, const int *factors, double *out);

/* ---- fixed nodes: poses held constant ------------------------------------------------------------------------------
 * A library-made xyt node (april_graph_node_xyt_create) is free or FIXED.  With Phi the fixed set, a step solves the normal equations with
 * the rows and columns of Phi removed: in the assembled system every block (i, j) with i or j in Phi is zero, every right-hand-side segment
 * of a node in Phi is zero and its diagonal block is exactly 1.0 * I (not 1 + tikhanov, not LM's lambda); a free node b keeps the whole
 * H_bb and g_b of a factor it shares with a fixed node.  dx and delta_X of a fixed node are +-0, its x and y come back bitwise unchanged.
 * Its heading passes through the state update's mod2pi like any other node's, (v + pi - 2 pi floor((v + pi) / 2 pi)) - pi: it is bitwise
 * unchanged exactly when that wrap returns it bitwise (true for most, not all, v in [-pi, pi)), and a heading outside [-pi, pi) comes
 * back wrapped.  With one node fixed a relative-only graph is regular at tikhanov = 0.  april_graph_chi2 and the LM / GNC objectives
 * still count every factor.
 * The flag lives in a tagged block on node->impl, which the reference leaves NULL on xyt nodes; the node's copy is deep, its destroy frees
 * the block.  .graph files do not store the flag: save ignores it, load returns free nodes.  A node keeps its place in the elimination
 * order, so fixing or freeing a node between two calls never re-plans; the next call of any kind sees the change.
 * Open to fixed nodes: april_graph_cholesky, aprilsam_amd_batch_resident and the resident loop, aprilsam_amd_optimize_lm and _gnc (their
 * damping never reaches a fixed node), aprilsam_amd_debug_stage, aprilsam_amd_solve (it solves the system that was factorised, identity
 * blocks included: x of a fixed node is its right-hand side), aprilsam_amd_marginals, _marginals_joint, _marginals_joint_any and
 * aprilsam_amd_gate_xyt: covariances of the free nodes are conditional on Phi, every row and column of a fixed node is exact zeros, so a
 * candidate between a new pose and a fixed map pose is gated with the new pose's covariance alone.  These consumers use the fixed set
 * the retained factor was made with; a toggle after the factorisation drops the retained factor and they answer as without one.
 * Refused with -12, nothing written: april_graph_cholesky_inc and _inc_solver (void: see aprilsam_amd_last_error; they look in the
 * reference's order, aprilsam.c:380-385 and 580: a param without a factorisation -- also one whose factor a consumer has dropped after a
 * toggle -- returns silently first, and so does april_graph_cholesky_inc on a graph without a factor the param has not seen),
 * aprilsam_amd_initialize_chordal, sharded params, aprilsam_amd_marginals_cross and aprilsam_amd_relative_covariances.
 * set_fixed: 0; -13 for a NULL node or a value other than 0 / 1; -12 when the node is not an xyt node of this library or node->impl is
 * in use by something else (node unchanged then).  set_fixed(node, 0) frees the block and leaves impl NULL. */
int aprilsam_amd_node_set_fixed(april_graph_node_t *node, int fixed);   /* 0 / 1 */
int aprilsam_amd_node_get_fixed(const april_graph_node_t *node);        /* 0 for any other node */

/* ---- graduated non-convexity: outlier-robust optimisation (Yang et al., RA-L 2020) ---------------------------
 * The robust losses above are non-convex and help only from a start near the optimum.  aprilsam_amd_optimize_gnc optimises a sequence of
 * surrogate losses on a list of CANDIDATE factors (typically every loop closure): the first almost quadratic, so the start does not
 * matter, the last Geman-McClure (GM) or truncated least squares (TLS).  With r the plain factor's residual (theta wrapped), s = r' W r,
 * the threshold c on sqrt(s), cc = c^2 and the control parameter mu:
 *     GM    m = mu cc:                       rho_mu(s) = m s / (m + s)                         w_mu(s) = (m / (m + s))^2
 *     TLS   lo = mu / (mu + 1) cc, hi = (mu + 1) / mu cc:
 *           s <= lo                          rho_mu(s) = s                                     w_mu(s) = 1
 *           s >= hi                          rho_mu(s) = cc                                    w_mu(s) = 0
 *           otherwise                        rho_mu(s) = 2 c sqrt(mu (mu + 1) s) - mu (cc + s)   w_mu(s) = c sqrt(mu (mu + 1) / s) - mu
 *           (mu = +inf: lo = hi = cc, TLS itself.)  w_mu = d rho_mu / d s.  A NaN s gives a NaN weight and a NaN rho.
 *   Start      s_max = the largest s over the candidates at the incoming states (a max reduction on the device).
 *              GM: mu_0 = max(1, 2 s_max / cc).  TLS: mu_0 = cc / (2 s_max - cc) when 2 s_max > cc; otherwise every candidate is an
 *              inlier: mu_0 = +inf, one stage with all weights 1 runs and the schedule is finished.
 *   Stage      exactly the iteration loop of aprilsam_amd_optimize_lm from the current x with opts.lm: lambda restarts at lambda0 and nu
 *              at 2; in the objective every candidate's term is rho_mu(s); at every linearisation every candidate's W_eff is
 *              w_mu(s) W, s taken where a robust factor's is (xyt: the l_points; xytpos: the node's state -- both x inside the run).
 *              Whatever LM status ends the stage, the run goes on (STALLED is counted in stages_stalled).
 *   Schedule   GM: after a stage stop if mu == 1 (status 1), else mu <- max(1, mu / mu_step).  TLS: after a stage evaluate the weights
 *              at the stage's final x; stop if all are exactly 0 or 1 (status 1), else mu <- mu * mu_step.  max_stages stages without
 *              that: status 2.
 *   mu lives in device memory and is written between stages; the ONE captured LM iteration is replayed for every stage.  The host
 *   synchronises once for s_max, once per lm.check_every iterations and (TLS) once per stage; results never depend on check_every, and
 *   two runs give identical bits.
 * Non-candidate factors keep their own behaviour inside the run: plain, robust and max factors as in aprilsam_amd_optimize_lm.
 * What the call leaves is what aprilsam_amd_optimize_lm leaves: state = l_point = x*, delta_X = the last accepted h (untouched if none), the
 * plan kept, the retained factor DROPPED, param->tikhanov untouched.  No factor object is modified: aprilsam_amd_factor_get_robust of a
 * candidate still says NONE, the packed W slots hold the plain W again, and a following april_graph_cholesky gives the bits it gives on a
 * fresh copy of the graph at the same states.
 * candidates: n distinct graph factor indices.  weights: NULL or n doubles, w_mu_final(s) of candidate i evaluated by a last device pass at
 * the returned states (not whatever the last linearisation used).  stage_trace: NULL or 4 * opts->max_stages doubles, one row per stage:
 * mu, F on entry under that mu, F at the stage's end, the stage's LM iterations.
 * Returns 0 (reason in report->status), or: -1 empty graph; -4 host-evaluated (foreign) factors; -12 sharded param, an asymmetric W
 * anywhere, or a candidate that is not a library-made xyt / xytpos factor, already carries a robust loss, is a max factor, or whose W is
 * not symmetric positive definite (all three leading minors > 0, mirror entries bitwise equal); -13 a null argument, n <= 0, an index out
 * of range, a duplicate index, bad options (loss, c, mu_step <= 1, max_stages < 1, anything aprilsam_amd_optimize_lm refuses in lm); -14
 * no HIP device.  On a refusal nothing is written and graph and param stay usable.  A failure during the run behaves as in
 * aprilsam_amd_optimize_lm.  aprilsam_amd_factor_set_robust keeps refusing kinds above 3: the surrogates are internal to the run. */
enum { APRILSAM_AMD_GNC_GM = 1, APRILSAM_AMD_GNC_TLS = 2 };
typedef struct {
    int    loss;          /* GM (default) or TLS */
    double c;             /* finite, > 0: threshold on the Mahalanobis distance sqrt(s); default sqrt(16.27), chi^2 of 3 dof at 0.999 */
    double mu_step;       /* > 1, default 1.4 */
    int    max_stages;    /* >= 1, default 100 */
    aprilsam_amd_lm_opts_t lm;   /* one stage's LM run; lm.max_iters is the cap PER STAGE, default 10 here; the rest as lm_opts_init */
} aprilsam_amd_gnc_opts_t;
void aprilsam_amd_gnc_opts_init(aprilsam_amd_gnc_opts_t *opts);
typedef struct {
    int    status;            /* 1 schedule finished (GM: the mu = 1 stage ran; TLS: every weight 0 or 1 after a stage), 2 max_stages */
    int    stages, iterations, accepted, stages_stalled;      /* iterations / accepted: LM iterations / accepted steps over all stages */
    int    n_inliers;         /* candidates with s <= c^2 at the returned states */
    double mu_initial, mu_final, s_max;
    double F_final;           /* the objective of the LAST stage at the returned states */
    double chi2_final;        /* april_graph_chi2 of the returned states (plain factors) */
} aprilsam_amd_gnc_report_t;
int aprilsam_amd_optimize_gnc(april_graph_t *graph, april_graph_cholesky_param_t *param, const aprilsam_amd_gnc_opts_t *opts,
                              int n, const int *candidates, aprilsam_amd_gnc_report_t *report, double *weights, double *stage_trace);
/* debug: hipGraphs captured and instantiated for this param so far (-1: no context; restarts when a failure drops the context) */
long long aprilsam_amd_debug_graph_captures(const april_graph_cholesky_param_t *param);

/* ---- multi-GPU: nested-dissection subtree sharding, one process per GPU -------
 * The reference has no counterpart (it is sequential); a C host drives a sharded solve through the same graph / param
 * objects it hands to april_graph_cholesky (aprilsam.h:268-281):
 *
 *     aprilsam_amd_shard_begin(graph, param, rank, world);            every rank, same graph: identical plans, fronts split
 *                                                                     over the ranks by proportional mapping of the assembly
 *                                                                     tree; THIS rank allocates only the fronts it owns plus
 *                                                                     "ghost" update blocks of children that live elsewhere
 *     aprilsam_amd_shard_comm_unique_id(id)  on rank 0, id sent to the other ranks by any means (file, socket, MPI, ...)
 *     aprilsam_amd_shard_comm_init_rccl(param, id);                   RCCL communicator over xGMI on the library's device
 *       -- or aprilsam_amd_shard_comm_init_host(param, &callbacks);   the caller moves pinned host buffers itself
 *     aprilsam_amd_shard_iterate(graph, param, n);                    n Gauss-Newton iterations; the exchange happens inside:
 *                                                                     per level, the Schur update of every front whose parent
 *                                                                     lives on another rank (packed lower trapezoid, point to
 *                                                                     point); on the way down the solved x of the "top"
 *                                                                     fronts (broadcast).  With RCCL everything is enqueued
 *                                                                     on the solver's HIP stream: no host synchronisation
 *                                                                     between a level's kernels and its transfers.
 *     aprilsam_amd_shard_chi2(graph, param);                          chi^2 of the whole graph (partial sums added); NaN when
 *                                                                     the call fails or the transport has failed, in this call
 *                                                                     or in an earlier one of the run (never this rank's partial
 *                                                                     sum); aprilsam_amd_last_error then holds -6 and the message
 *     aprilsam_amd_shard_gather_states(graph, param);                 every rank ends up with ALL states / l_points / dx,
 *                                                                     in HBM and in the node objects
 *     aprilsam_amd_shard_end(param);
 *
 * No all-reduce on the data path; world = 1 needs no transport.
 *   shard_info what: 0 -> {levels, fronts, nodes, pool doubles of this rank, pool doubles of the whole plan};
 *                    1 -> transfers {level, front, src, dst, (unused), packed count in doubles};
 *                    2 -> broadcasts {level, front, owner, first position, blocks}; 3 -> owner rank per front;
 *                    4 -> modelled critical path in sum c_j^2 flops {whole factorisation, heaviest root path through the fronts that
 *                         span several ranks (each runs on one owner), the busiest rank's own subtrees, all such fronts together}:
 *                         speed-up bound = [0] / ([1] + [2])
 * Return codes: 0 ok; -1 bad arguments / no shard_begin; -2 non-positive pivot; -4 foreign factor types; -5 librccl.so not
 * loadable; -6 communication error (RCCL or host callback; message on stderr); -7 no transport attached. */
typedef struct aprilsam_amd_host_comm {
    void *user;                                                           /* passed back to every callback */
    int (*send)(void *user, const double *buf, long long count, int dst);           /* blocking; 0 = ok */
    int (*recv)(void *user, double *buf, long long count, int src);
    int (*bcast)(void *user, double *buf, long long count, int root);               /* in place */
    int (*allreduce_sum)(void *user, double *buf, long long count);                 /* in place */
} aprilsam_amd_host_comm_t;
int       aprilsam_amd_shard_begin(april_graph_t *graph, april_graph_cholesky_param_t *param, int rank, int world);
long long aprilsam_amd_shard_info(const april_graph_cholesky_param_t *param, int what, long long *out, long long cap);
int       aprilsam_amd_shard_comm_unique_id(char *out128);
int       aprilsam_amd_shard_comm_init_rccl(april_graph_cholesky_param_t *param, const char *id128);
int       aprilsam_amd_shard_comm_init_host(april_graph_cholesky_param_t *param, const aprilsam_amd_host_comm_t *callbacks);
/* the attached transport as the communication library reports it: out5 = {kind (0 none, 1 RCCL, 2 host callbacks),
 * ncclCommCount, ncclCommUserRank, ncclGetVersion code, HIP device}; rccl_path (may be NULL): the librccl file in use */
int       aprilsam_amd_shard_comm_info(const april_graph_cholesky_param_t *param, long long *out5, char *rccl_path, int cap);
int       aprilsam_amd_shard_iterate(april_graph_t *graph, april_graph_cholesky_param_t *param, int n);
int       aprilsam_amd_shard_gather_states(april_graph_t *graph, april_graph_cholesky_param_t *param);
double    aprilsam_amd_shard_chi2(april_graph_t *graph, april_graph_cholesky_param_t *param);
void      aprilsam_amd_shard_end(april_graph_cholesky_param_t *param);

/* ---- host-logic introspection (no GPU needed): ordering + symbolic analysis of a graph -------- */
typedef struct aprilsam_amd_plan aprilsam_amd_plan_t;   /* opaque */
aprilsam_amd_plan_t *aprilsam_amd_plan_create(int n_nodes, int n_factors, const int *factor_nodes /* 2 per factor, -1 for unary */,
                                              const double *xy /* 2 per node or NULL */, int leaf_nodes);
void aprilsam_amd_plan_destroy(aprilsam_amd_plan_t *plan);
/* query: fills *out with a malloc'ed int64 array the caller frees with aprilsam_amd_free(); returns its length.
 * what: "perm" (position->node), "front_ptr" , "front_nsb", "front_nub", "front_parent", "front_level",
 *       "front_rows_ptr", "front_rows" (block positions of every front's rows: own then struct),
 *       "factor_front", "stats" (n_fronts, n_levels, max_rows, nnzL, flops) */
long long aprilsam_amd_plan_query(const aprilsam_amd_plan_t *plan, const char *what, long long **out);
/* Ownership map and exchange lists of a `world`-rank sharded run of this plan, as aprilsam_amd_shard_info reports them
 * (what: 1 transfers x6, 2 broadcasts x5, 3 owner per front, 4 modelled critical path x4); host logic only. */
long long aprilsam_amd_shard_plan(const aprilsam_amd_plan_t *plan, int world, int what, long long *out, long long cap);
/* XCD placement of the batch step's multi-level launches for an assembly tree (parent, level, own pose blocks per front): the fronts
 * of levels >= l0 (and, when l0 == 1, the level-0 leaves) as padded workgroup lists, -1 = empty slot.  which: 0 up-sweep list,
 * 1 down-sweep list, 2 leaf list (returns the length; fills out up to out_cap), 3 the self-check (0 or a negative code); host logic only. */
int aprilsam_amd_xcd_place(int nF, const int *parent, const int *level, const int *nsb, int l0, int cap, int cap_leaf, int which, int *out, int out_cap);
/* The same tree's back substitution list when level 0 joins the multi-level launch that starts at level 1 (option "persist_leaves"): the
 * upper fronts' slots unchanged, then the leaves.  which: 0 level order, 1 XCD-placed (down-sweep list, then leaf list), 2 / 3 the self-check of
 * 0 / 1 (0 or a negative code); host logic only. */
int aprilsam_amd_persist_leaves_list(int nF, const int *parent, const int *level, const int *nsb, int cap, int cap_leaf, int which, int *out, int out_cap);
/* The order of the factorisation's one launch (option "persist_up").  base: the launch's list in level order, children before parents, -1 in
 * empty slots, a front's class being its slot % 8 (for a tree whose multi-level launches start at level 1: aprilsam_amd_xcd_place's leaf list
 * followed by its up-sweep list).  mode 0 / 1: base itself, 2: descending priority, 3: the slot-aware list schedule with cap slots per class.
 * which: 0 the list (returns the length; fills out up to out_cap), 1 the self-check of the list against base (0 or a negative code).
 * makespan (may be NULL) receives the cost model's makespan of the returned list in us, so mode 0 gives that of any list; host logic only. */
int aprilsam_amd_up_schedule(int nF, const int *parent, const int *nsb, const int *base, int n_base, int cap, int mode, int which, int *out, int out_cap, double *makespan);
/* Which wave of a front's workgroup adds its children's update blocks into which block column (option "asm_balance").  A tree of nF fronts
 * (children have lower indices than their parents; parent -1: a root); front t has nsb[t] own and nub[t] update blocks, and entry
 * rows_ptr[t] + j of rel (aprilsam_amd_plan_query: "front_rows_ptr", "front_rel") is the block column of t's parent that t's update block j
 * goes to.  owner (rows_ptr[nF] ints) receives for every such entry the wave, 0 .. nw - 1, that owns its column in the parent: per parent the
 * columns are taken by decreasing number of work items (one per child block, one more where 3 nub + 1 - 3 j > 64) and each goes to the least
 * loaded wave, ties to the lower column and then the lower wave; -1 for the entries of a root.  A parent whose longest list would come out
 * longer that way than with column b on wave b mod nw keeps b mod nw for all its columns (longest-first is a heuristic), so no parent's
 * longest list is ever longer than under the modulo rule.  Returns 0, or -100 for arguments that are no such tree (rows_ptr must start at
 * 0 or above and advance by nub[t]); host logic only. */
int aprilsam_amd_asm_owners(int nF, const int *parent, const int *nsb, const int *nub, const long long *rows_ptr, const int *rel, int nw, int *owner);
void aprilsam_amd_free(void *p);

/* Host logic behind the incremental path: the reference's elimination order (aprilsam.c:999-1249, restated
 * with its tie-breaking) and the block elimination tree it implies (aprilsam.c:613-657).  fb[i] < 0 marks a
 * unary factor.  out_order: position -> node; out_parent (may be NULL): node -> parent node or -1. */
int aprilsam_amd_reference_order(int n_nodes, int n_factors, const int *fa, const int *fb, int *out_order, int *out_parent);

/* test handle on the same bookkeeping model, stepped explicitly (see tests/test_refmodel.py) */
void *aprilsam_amd_refmodel_create(void);
void  aprilsam_amd_refmodel_destroy(void *m);
void  aprilsam_amd_refmodel_batch(void *m, int n_nodes, int n_factors, const int *fa, const int *fb);
int   aprilsam_amd_refmodel_inc_begin(void *m, int n_nodes, int n_factors, const int *fa, const int *fb);   /* -> naffected */
int   aprilsam_amd_refmodel_solve_visit(void *m, const double *x, double dxy, double dth, int *visited);    /* -> start_over */
void  aprilsam_amd_refmodel_get(void *m, int *parent, int *changed, int *relin);
int   aprilsam_amd_refmodel_check(void *m);   /* 0: the incrementally maintained tree equals a full recomputation */

/* ---- synthetic Manhattan lattice generator ----------------------- */
/* Appends K*K xyt nodes, the in-bounds 4-direction xyt factors and the node-0 prior to `graph`.
 * Returns the number of factors added. */
int aprilsam_amd_make_lattice(april_graph_t *graph, int K);
/* The same lattice as plain arrays: states[3*K*K], fa/fb[F] (fb = -1 for the prior), z[3F], W[9F] with
 * F = 2K(K-1) + 2(K-1)^2 + 1 (caller allocates).  Returns F. */
int aprilsam_amd_lattice_arrays(int K, double *states, int *fa, int *fb, double *z, double *W);
/* Bulk append N xyt nodes (state = init = truth) and F factors (fb[i] < 0: xytpos prior on fa[i]). */
void aprilsam_amd_graph_from_arrays(april_graph_t *graph, int N, const double *states, int F, const int *fa,
                                    const int *fb, const double *z, const double *W);

/* Bulk read of the node objects: state / l_point / delta_X of every node (3 doubles each, node order; any destination may
 * be NULL).  Assumes xyt nodes (3 degrees of freedom), like the two calls above. */
void aprilsam_amd_graph_node_arrays(const april_graph_t *graph, double *state, double *l_point, double *delta_X);

/* Stage-level parity exports (tests/test_gpu_stages.py): the device linearisation and the gather assembly seen in the
 * caller's node coordinates, at the graph's current states (l_point <- state first, as a batch step does).
 *   what 0: out[33 * F], per factor (J_a^T W) J_a, (J_a^T W) J_b, (J_b^T W) J_b (3 x 3 row-major each), (J_a^T W) r, (J_b^T W) r
 *           -- the products the reference forms at aprilsam.c:159-192 from april_graph_xyt.c:62-124 / april_graph_xytpos.c:63-102
 *   what 1: out[9 N^2 + 3 N]: A = sum J^T W J + tikhanov * I (dense, symmetric, row-major) then B = sum J^T W r, both in
 *           node order -- param->A (un-permuted) and param->B of aprilsam.c:159-204; N <= 2000
 * Returns 0, or < 0 (empty graph, foreign factor types, too large). */
int aprilsam_amd_debug_stage(april_graph_t *graph, april_graph_cholesky_param_t *param, int what, double *out);

/* debug (env APRILSAM_AMD_KPROF=1): 16 wall-clock stamps (100 MHz ticks) per front from the last numeric pass */
int aprilsam_amd_debug_front_times(const april_graph_cholesky_param_t *param, long long *out, int n_fronts);

/* debug (tests/test_gpu_front_shapes.py): the form every front of the param's batch plan takes in a batch step's launches under the options
 * the plan was made with, read from the launch tables themselves -- nothing is decided again.  out (ints):
 *   [0] fronts nF   [1] levels   [2] ints per front (8)   [3] offset of the level records
 *   per front t, at 4 + 8 t: level; factorisation 0 full-LDS / 1 panel / 2 multi-workgroup; 1 = inside the multi-level launch of the
 *     up-sweep; the same of the down-sweep; back substitution 0 k_backsolve_w / 1 k_backsolve_t / 2 k_backsolve_t TALL / 3 k_backsolve_blk;
 *     helper workgroups of k_backsolve_blk; 1 = k_backsolve_gemv precedes it; hand-over form of its down launch (0 flush, 1 write-through,
 *     2 granules; -1: its launch follows a kernel boundary)
 *   per level, from [3] on: fronts on the multi-workgroup path; 1 = wide updates grouped; outer blocks nob; then nob x { rb of k_block_solve,
 *     tile of the wide update that closes the block, of the "ahead" update, of the single-block update; 0 = no such launch }
 * Returns the number of ints the record takes (out is filled up to cap), or -1: no plan, or a plan extended by tail fronts. */
int aprilsam_amd_debug_front_forms(const april_graph_cholesky_param_t *param, int *out, int cap);

/* debug (tests/test_gpu_inc_shapes.py): what the param's most recent april_graph_cholesky_inc did, noted by the host code of the incremental
 * path at the places where it decides these things -- read-only, nothing is decided again.  out (ints):
 *   [0] rows (dirty fronts)   [1] ints of this header (14)   [2] ints per row (14)
 *   [3] path: 0 full re-plan; 1 tail_refactor inside k_inc_one, back substitution in its window (solve_here); 2 the same with a list of
 *       fronts to back-substitute; 3 tail_refactor on the general path; 4 general step as one k_inc_one; 5 multi-level launch; 6 per-level launches
 *   [4] for a re-plan, the exit of inc_fast_step it left by (0: the fast path was not tried)   [5] new factors of the step
 *   [6] [7] [8] [9] the tail step's a_idx, n_old, n_new, s_idx (-1: no tail_refactor; s_idx -1: no solve in the window)
 *   [10] workgroup size of the step's (first) front launch   [11] 1 = the whole step was one k_inc_one launch
 *   [12] 1 = fronts in a multi-level launch of their own   [13] 1 = back substitution in a multi-level launch of its own
 *   per dirty front, children before parents: front id; mode 1 low-rank updated / 0 re-assembled (or its trailing columns refactorised);
 *     own pose blocks nsb; update blocks nub after the step; nub before it; the step's factor slots the front sees (bit mask; updated fronts);
 *     own new factors taken as slots; updated children; 1 = its array was rewritten in place; 1 = its structure gained a row that is not
 *     its last (mid); then the update blocks of each updated child (4 ints, -1 = none)
 * Returns the number of ints the record takes (out is filled up to cap), or -1: no incremental call on this param yet. */
int aprilsam_amd_debug_inc_forms(const april_graph_cholesky_param_t *param, int *out, int cap);

const char *aprilsam_amd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* APRILSAM_AMD_H */
