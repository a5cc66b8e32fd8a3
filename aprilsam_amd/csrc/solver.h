// solver.h — internal interface between the C-ABI layer (capi.cpp) and the HIP runtime (solver.hip.cpp)
#pragma once
#include <vector>
#include "../../include/aprilsam_amd.h"

namespace asam {

struct Options {
    int leaf_nodes = 16;          // nested-dissection leaf size (pose nodes)
    int deterministic = 0;        // 1: the wall-clock fallback rule aprilsam.c:557-559 is disabled (0 = the reference's behaviour)
    int use_graph = 1;            // replay the numeric phase from a captured hipGraph
    int device_timing = 0;        // record HIP events per stage (disables graph replay for that call)
    int trust_factor_cache = 0;   // 1: z/W of factors already packed are treated as immutable (skips the per-call content check)
    int small_lds_kb = 156;       // fronts whose LDS image fits run in the single-workgroup LDS kernel
    int inc_fast = 1;             // incremental steps regenerate only the dirty root paths (0: full re-plan per step)
    int inc_multi = 1;            // incremental steps: the regenerated fronts of all levels as ONE multi-level launch, the back substitution as another (0: one launch per level)
    int inc_one = 1;              // ... and a step that regenerates at most inc_one_up fronts and walks at most inc_one_dn as ONE single-workgroup launch
    int inc_one_up = 3, inc_one_dn = 4, inc_one_threads = 512, inc_one_spin = 1;
    int inc_tail = 1;             // ... and steps whose factors touch the last few poses of the last tail front alone re-factorise its trailing columns only
    int inc_inline = 1;           // ... a small step's table / factor / state patches travel in the kernel arguments instead of being read across PCIe
    int inc_tail_solve = 1;       // ... and when every pose the step's walk visits lies among those trailing columns, the back substitution and the state update happen in the same LDS window
    int inc_lazy_states = 1;      // ... and a step whose walk is partial compares only the node objects it reads (poses of its new factors, visited poses) with the state mirrors, not all of them
    int inc_replan_tall = 1;      // ... and when a front of an all-single-workgroup plan outgrows the LDS (rows collected from loop closures), the step re-plans instead of taking the multi-launch path from then on
    int inc_update = 1;           // ... and the fronts on the root path of a loop closure take a low-rank UPDATE of their factor (front_update_body) instead of being re-assembled and re-factorised
    int speculate_factors = 1;    // warm batch calls: the pass over the factor objects (edits in place) runs under the GPU's work on the packed copies; an edit voids the run
    int warm_up = 1;              // april_graph_cholesky_param_init initialises the HIP runtime's lazy parts once per process (a stream, the copy engines' queues, the code object, the graph machinery) instead of the first solver calls; 0 = leave them lazy (APRILSAM_AMD_WARM_UP=0: the option is read from the environment before the first param exists)
    int syrk_xcd_order = 512;     // wide trailing updates of at least this many tiles (one round of workgroups is 512): tile order in which every XCD works on 8 x 8 blocks of tiles (kernels.hip.h: trapezoid_tile_xcd); 0 = never
    int syrk_small_tiles = 320;   // wide trailing updates of fewer 64 x 64 tiles than this (a quarter of a round of workgroups) use 32 x 32 tiles; 0 = never.  Measured on the 100 k lattice: k_syrk_big 0.664 (never) / 0.633 (320) / 0.648 (640) / 0.676 (1280) ms -- such a launch is 27 us of start / end latencies whatever its tiles
    int syrk_pair_tiles = 2048;   // big fronts: levels whose first wide update has at least this many 64 x 64 tiles close every PAIR of outer blocks with one K = 256 update (after the first block of a pair only the next block's columns are updated); 0 = never.  Smaller updates are a launch's worth of latency whatever their K: pairs only add a launch there
    int syrk_group = 3;           // ... outer blocks per group (2: pairs, K = 256; 3: K = 384 -- measured best on the 1 M lattice: k_syrk_big 14.9 -> 13.1 (2) -> 12.75 (3) -> 12.9 ms (4, 6); inside a group the next block's columns are updated left-looking with K = the group's blocks so far)
    int schur_first = 40;         // panel-mode small fronts with at least this many update blocks: update columns assembled after the Schur product has been stored into them (0 = never; M3500's fronts stay below: on its latency path the second assembly pass costs more than the zero fill it saves)
    int small_threads = 1024;     // workgroup size of k_front_small (256 / 512 / 1024) on latency-bound levels ...
    int tp_threads = 512;         // ... and on throughput levels (>= tp_fronts fronts)
    int tp_fronts = 1000;         // levels with at least this many fronts are "throughput levels" ...
    int tp_lds_kb = 80;           // ... where only fronts up to this LDS size run fully in LDS (the rest: panel mode, more workgroups per CU).  80 KB = two such workgroups per compute unit; measured, round 6, k_front_small ms per iteration at 48 / 64 / 80 / 96 / 160: 100 k lattice 0.976 / 0.936-0.955 / 0.924-0.936 / 1.174 / 1.100, 1 M lattice 8.65 / 8.22-8.36 / 7.94-8.05 / 10.98 / 10.59
    int amalg = 0;                // 1 = separator amalgamation (symbolic.cpp: amalgamate): separator fronts take in child separators where a cost model of the critical path (hand-over per front vs pivot chain per column) says so -- fewer dependent levels on graphs the size of M3500
    int amalg_max = 64;           // ... as long as the merged front owns at most this many poses
    int pin_last = 0;             // nested dissection keeps the pin_last newest poses out of the dissection: they form the root front ("recent poses last")
    int batch_extend = 1;         // batch calls on a graph that only grew reuse the plan: appended poses become tail fronts, every front is re-factorised
    int extend_tail_fronts = 3;   // ... until the appended poses are this many tail fronts' worth, units of 24 poses (then: full re-plan).  Measured, round 4: demo --batch_update_only 1 500 poses 481 / 388 / 372 / 371 ms at 8 / 4 / 3 / 2; the incremental demo does not care (510 +- 3 %)
    int persist = 1;              // batch path: the top levels of the tree (few small fronts each) as ONE launch per sweep, fronts synchronised by dependency flags
    int persist_max_fronts = 240; // ... as many top levels as fit this many fronts
    int persist_leaves = 1;       // ... and level 0 inside the back substitution's launch where only persist_max_fronts kept it out (upload_plan has the rule): the leaves wait for their parents' x with their L panel in LDS, one k_backsolve_w per step instead of two; 0 = level 0 keeps its own launch.  Measured on M3500: hop into level 0 10-16 -> 0.7 us, resident step 0.2026 -> 0.1978 ms median (profiles/persist_leaves.txt); the up-sweep's half: persist_up
    int persist_up = 2;           // ... and level 0 inside the factorisation's launch under the same rule, where no front changes between its full-LDS and its panel form (upload_plan): 0 = its own launch; 1 = joined, level order; 2 = joined, descending remaining path to the root's end (a cost model's critical path is dispatched first); 3 = joined, the slot-aware list schedule (plan.h: up_schedule); 2 and 3 also order the one launch of graphs that never had two.  Measured on M3500, eight alternating runs against the parent commit: resident step 0.19808 -> 0.19570 (1) / 0.18774 (2) / 0.18812 ms (3) median, -5.2 % for 2, every run of 2 below every parent run; 2 and 3 cannot be told apart, the simpler one is the default (profiles/persist_up.txt)
    int xcd_place = 1;            // ... and their lists (and those of the level-0 launches below them) in an order where a front shares its costliest child's XCD (plan.h: xcd_place); 0 = level by level.  Measured on M3500: 0.2131 -> 0.2102 ms (the back substitution's two launches alone: 0.2113)
    int asm_balance = 1;          // extend-add of the small fronts: a parent's block columns are given to its workgroup's waves by item count, longest first to the least loaded wave (plan.h: asm_owners), instead of column mod waves; 0 = modulo everywhere.  The sums keep their order either way: the results are bitwise equal
    int tail_poses = 28;          // incremental path: own poses per tail front (>= 8; measured on the M3500 demo: 24 / 28 / 32 -> 546 / 530 / 528 ms total, median 0.038 / 0.0385 / 0.040 ms)
    int blk_backsolve = 1;        // wide multi-workgroup fronts: back substitution 128 columns at a time by a chain workgroup + helpers (0: k_backsolve_gemv + k_backsolve_t)
    int wave_backsolve = 1;       // multi-level back substitution: column-per-lane kernel (0: the per-32-column-block kernel)
    int tagged_x = 1;             // multi-level back substitutions: how a front hands its x to its children.  1 = as epoch-tagged 16-byte granules, no flag (kernels.hip.h: gather_x; a launch holding a front of more than 256 update rows takes form 2: launch_xmode); 0 = write-through x, drained, then the flag -- no L2 write-back (publish_flag_wt); 2 = plain x, L2 write-back, flag (publish_flag: the form before, kept for measurements).  Measured on M3500, resident step: 0.2092 (2 and the commit before) / 0.2093 (0) / 0.2028 ms (1), profiles/r08_downsweep_handover.txt
    int linearize_staged_min = 32768; // factors per launch from which k_linearize writes its results out through LDS (coalesced stores)
    int mem_cap_mb = 0;           // > 0: refuse any single device buffer above this size with ERR_OOM (tests: the out-of-memory path)
    int solve_chunk_cols = 0;     // aprilsam_amd_solve: columns per chunk of the work buffer, rounded up to a multiple of 16 (0 = as many as keep the buffer under 1 GB / mem_cap_mb, at least 16); the results do not depend on it
    int pool_guard = 0;           // debug: > 0 = every frontal array of a plan is followed by a guard band of this many doubles, NaN-filled at plan upload and checked after every synchronised step (ERR_GUARD); a stray read that is used poisons the result
    int pool_poison = 0;          // debug: 1 = before every step, the update block of every front the step (re)factorises and x at its own positions are filled with NaN: a dependency wait of a multi-level launch that passes early yields NaN instead of the previous step's numbers
    int skip_flag_waits = 0;      // debug, negative control of pool_poison: 1 = the fronts of the batch path's multi-level factorisation launch do NOT wait for their children
    int polar_on_host = 0;        // debug: 1 = polar factors are packed as host-evaluated foreign factors through their own eval() (the A/B oracle of the native path)
    int gaussian_on_host = 0;     // debug: 1 = dense Gaussian factors are packed as host-evaluated cliques through their own eval() (the A/B oracle of the native path)
    int panel_mode = 1;           // fronts too large for LDS whose own columns fit run in k_front_small's panel mode
};
extern Options g_opt;

void batch_step(april_graph_t *g, april_graph_cholesky_param_t *param);
void inc_step(april_graph_t *g, april_graph_cholesky_param_t *param);
void inc_solve_only(april_graph_t *g, april_graph_cholesky_param_t *param);
double graph_chi2(april_graph_t *g);
int batch_resident(april_graph_t *g, april_graph_cholesky_param_t *param, int iters, double *chi2_out, double *ms_out);
int resident_begin(april_graph_t *g, april_graph_cholesky_param_t *param);
int resident_steps(april_graph_t *g, april_graph_cholesky_param_t *param, int n, int mode);
int resident_sync(april_graph_t *g, april_graph_cholesky_param_t *param);
double resident_chi2(april_graph_t *g);
int resident_end(april_graph_t *g, april_graph_cholesky_param_t *param);
int level_profile(const april_graph_cholesky_param_t *param, double *out, int cap_levels);
int debug_front_forms(const april_graph_cholesky_param_t *param, int *out, int cap);
int debug_inc_forms(const april_graph_cholesky_param_t *param, int *out, int cap);
int kernel_profile(const april_graph_cholesky_param_t *param, double *ms, long long *calls, double *flops, double *bytes, const char **names);
void drop_context(const april_graph_cholesky_param_t *p);
void drop_graph_pack(const april_graph_t *g);
bool get_stats(const april_graph_cholesky_param_t *p, aprilsam_amd_stats_t *out);
int shard_begin(april_graph_t *g, april_graph_cholesky_param_t *param, int rank, int world);
long long shard_info(const april_graph_cholesky_param_t *param, int what, long long *out, long long cap);
int shard_comm_unique_id(char *out128);
int shard_comm_init_rccl(const april_graph_cholesky_param_t *param, const char *id128);
int shard_comm_init_host(const april_graph_cholesky_param_t *param, const aprilsam_amd_host_comm_t *cb);
int shard_comm_info(const april_graph_cholesky_param_t *param, long long *out, char *path, int cap);
int shard_iterate(april_graph_t *g, april_graph_cholesky_param_t *param, int n);
int shard_gather_states(april_graph_t *g, april_graph_cholesky_param_t *param);
double shard_chi2(april_graph_t *g, april_graph_cholesky_param_t *param);
void shard_end(const april_graph_cholesky_param_t *param);
int debug_guard_selftest(const april_graph_cholesky_param_t *param);
int debug_stage(april_graph_t *g, april_graph_cholesky_param_t *param, int what, double *out);
int debug_front_times(const april_graph_cholesky_param_t *param, long long *out, int n_fronts);
int api_device_count();
int selftest();
struct Plan;
void shard_map(const Plan &P, int world, std::vector<int> &owner, std::vector<char> &top, std::vector<long long> &xfer, std::vector<long long> &bcast);
std::vector<long long> shard_critical_path(const Plan &P, int world, const std::vector<int> &owner, const std::vector<char> &top);
int api_set_device(int d);
int api_param_set_device(const april_graph_cholesky_param_t *param, int slot);
int api_param_get_device(const april_graph_cholesky_param_t *param);
void unbind_param(const april_graph_cholesky_param_t *param);
void warm_up() noexcept;          // once per process, from april_graph_cholesky_param_init: see solver.hip.cpp
int api_set_option(const char *name, double v);
int api_get_option(const char *name, double *v);
int marginals(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *qa, const int *qb, double *cov, bool joint);     // solver_marginals.inc.h
long long selinv_runs(const april_graph_cholesky_param_t *param);
int marginals_joint_any(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, double *cov);      // solver_gating.inc.h
int gate_xyt(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, const double *z, const double *W, double *d2, double *S);
int marginals_set(april_graph_t *g, april_graph_cholesky_param_t *param, int k, const int *nodes, double *cov);
int gate_xyt_joint(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b, const double *z,
                   const double *W, double *d2_prefix, double *C);
int gate_polar(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *a, const int *b, const int *kind, const double *z, const double *W,
               double *d2, double *S);
int associate_polar(april_graph_t *g, april_graph_cholesky_param_t *param, int observer, int m, const int *kind, const double *z, const double *W, int L,
                    const int *landmarks, double gate1, double gate2, double *d2, int *best, double *d2_best, double *d2_second);
long long path_solve_bytes(const april_graph_cholesky_param_t *param);
int logdet(april_graph_t *g, april_graph_cholesky_param_t *param, double *out);                                                      // solver_info.inc.h
int logdet_sets(april_graph_t *g, april_graph_cholesky_param_t *param, int n_sets, const int *set_ptr, const int *nodes, double *logdet_prefix);
int info_gain_xyt(april_graph_t *g, april_graph_cholesky_param_t *param, int n_hyp, const int *hyp_ptr, const int *a, const int *b, const double *W,
                  double *gain_prefix);
int tree_solve(april_graph_t *g, april_graph_cholesky_param_t *param, int mode, int nrhs, const double *B, double *X);                // solver_treesolve.inc.h
int marginals_cross(april_graph_t *g, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov);
int relative_covariances(april_graph_t *g, april_graph_cholesky_param_t *param, int anchor, int n, const int *nodes, double *cov);
long long tree_solve_bytes(const april_graph_cholesky_param_t *param);
int factorised_nodes(const april_graph_cholesky_param_t *param);
int max_selected(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *factors, int *out);   // solver_pack.inc.h
void lm_opts_init(aprilsam_amd_lm_opts_t *opts);                                                                    // solver_lm.inc.h
int optimize_lm(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_lm_opts_t *opts, aprilsam_amd_lm_report_t *report, double *trace);
void gnc_opts_init(aprilsam_amd_gnc_opts_t *opts);                                                                  // solver_gnc.inc.h
int optimize_gnc(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_gnc_opts_t *opts, int n, const int *candidates,
                 aprilsam_amd_gnc_report_t *report, double *weights, double *stage_trace);
long long graph_captures(const april_graph_cholesky_param_t *param);                                               // solver_launch.inc.h
void chordal_opts_init(aprilsam_amd_chordal_opts_t *opts);                                                         // solver_chordal.inc.h
int initialize_chordal(april_graph_t *g, april_graph_cholesky_param_t *param, const aprilsam_amd_chordal_opts_t *opts, aprilsam_amd_chordal_report_t *report,
                       double *rot_out, double *raw_out);
// max-mixture factors (host_objects.cpp)
constexpr int MAX_MIX_K = 8;
bool is_native_max(const april_graph_factor_t *f);                 // type 3 with this library's eval
bool max_check(const april_graph_factor_t *f, char *why, int cap);  // component count, types, endpoints, symmetric W with det > 0, finite logw
double max_const(const april_graph_factor_t *f, int i);           // -2 logw_i - ln det W_i
int max_select(const april_graph_factor_t *f, const double *pa, const double *pb);
// robust losses (host_objects.cpp): true for a library xyt / xytpos factor that carries one, with its kind and c
bool robust_of(const april_graph_factor_t *f, int *kind, double *c);
bool plain_common_factor(const april_graph_factor_t *f);           // an xyt / xytpos factor made by this library, with its z and W in place (it may carry a loss)
double robust_host_s(const double *z, const double *w, const double *pa, const double *pb);      // r^T W r at pa (/ pb: xyt), eval_finish's association
// range / bearing / range-bearing factors (host_objects.cpp): true for this library's polar factor, with its kind
bool polar_of(const april_graph_factor_t *f, int *kind);
// dense Gaussian factors (host_objects.cpp): true for this library's Gaussian factor, with its node count, its chi^2
// constant c0 and whether eta / Lambda (as they stand now: edited in place, they are factorised again here) are admissible
bool gaussian_of(const april_graph_factor_t *f, int *k, double *c0, bool *ok);
bool gaussian_ever();                                            // false until the process makes its first Gaussian factor: graphs are not walked for them before
// fixed nodes (host_objects.cpp): true for an xyt node of this library that is held constant
bool node_fixed(const april_graph_node_t *n);
bool fixed_ever();                                               // false until the process fixes its first node: graphs are not walked for flags before
int robust_weights(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *factors, double *w);   // solver_calls.inc.h
int factor_audit(april_graph_t *g, april_graph_cholesky_param_t *param, int n, const int *factors, double *out);   // solver_audit.inc.h
int marginal_prior(april_graph_t *g, april_graph_cholesky_param_t *param, int m, const int *remove, int cap, int *n_keep, int *keep, double *xbar, double *eta,
                   double *Lambda);                                                                                 // solver_marginal_prior.inc.h
int graph_marginalize(april_graph_t *g, april_graph_cholesky_param_t *param, int m, const int *remove, int *new_index);

}  // namespace asam
