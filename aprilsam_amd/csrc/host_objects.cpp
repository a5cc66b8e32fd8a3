// host_objects.cpp — host-side graph objects with the reference's ABI (include/aprilsam_amd.h PART 1/3).
//
// These constructors let a caller build a graph without libaprilsam: objects are laid out exactly like
// the reference's (april_graph.c:329-364, april_graph_xyt.c:276-298,420-438, april_graph_xytpos.c:191-211)
// and carry working vtable entries (copy / eval / state_eval / destroy, update / relinearize / destroy)
// because reference-compiled host code calls them directly (examples/aprilsam_demo.c:183 nb->relinearize,
// :166 exist_factor->copy, april_graph.c:335-346 ->destroy).  The vtable entries are a courtesy to such
// callers; the solver entry points never call them — factors of type 1/2 are evaluated by the HIP
// kernels (csrc/kernels.hip.h).  Max-mixture factors (type 3) are built here too: their selection rule
// (max_select) is the one the incremental path applies on the host and k_select_mixture restates on the device.  Robust losses on xyt /
// xytpos factors are kept here as well: a tagged block hung off u.common.impl, applied by eval_finish.  Range, bearing
// and range-bearing factors (type 4) are built here: true m-row factors on the host, xyt slots on the device (polar.h).
// Dense Gaussian factors on k nodes (type 5) and the graph edit that removes nodes are here as well: the factor's
// square-root form (a pivoted Cholesky) is what its host evaluation returns; the device takes Lambda and eta as they are (gaussian.hip.h).
#include <atomic>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>
#include <cstdlib>
#include <cstring>

#include "../../include/aprilsam_amd.h"
#include "solver.h"
#include "errors.h"
#include "robust.h"
#include "polar.h"

namespace {

double *dup3(const double *v) {              // doubles_dup (doubles_floats_impl.h:68), NULL-tolerant
    if (!v) return nullptr;
    double *r = (double *)malloc(3 * sizeof(double));
    memcpy(r, v, 3 * sizeof(double));
    return r;
}
matd_t *matd33(const double *data) {
    matd_t *m = (matd_t *)calloc(1, sizeof(matd_t) + 9 * sizeof(double));
    m->nrows = 3; m->ncols = 3;
    if (data) memcpy(m->data, data, 9 * sizeof(double));
    return m;
}
double mod2pi_h(double v) {                   // math_util.h:113-122
    const double TWOPI = 6.2831853071795862319959, PI_ = 3.141592653589793238462643383279502884196;
    double vin = v + PI_;
    return (vin - TWOPI * floor(vin / TWOPI)) - PI_;
}
void zarray_append(zarray_t *za, const void *p) {      // zarray.h:152-189 semantics (doubling growth)
    if (za->size + 1 > za->alloc) {
        int na = za->alloc;
        while (na < za->size + 1) { na *= 2; if (na < 8) na = 8; }
        za->data = (char *)realloc(za->data, (size_t)na * za->el_sz);
        za->alloc = na;
    }
    memcpy(za->data + (size_t)za->size * za->el_sz, p, za->el_sz);
    za->size++;
}
zarray_t *zarray_new(size_t el_sz) {
    zarray_t *za = (zarray_t *)calloc(1, sizeof(zarray_t));
    za->el_sz = el_sz;
    return za;
}

april_graph_factor_eval_t *eval_alloc(int njac) {
    april_graph_factor_eval_t *e = (april_graph_factor_eval_t *)calloc(1, sizeof(*e));
    e->jacobians = (matd_t **)calloc(njac + 1, sizeof(matd_t *));      // NULL-terminated
    for (int i = 0; i < njac; i++) e->jacobians[i] = matd33(nullptr);
    e->r = (double *)calloc(3, sizeof(double));
    e->W = matd33(nullptr);
    return e;
}
// ---- robust loss ----------------------------------------------------------------------
// The reference leaves u.common.impl unused (NULL) for its xyt / xytpos factors.  A library factor with a loss points it at this block;
// the tag tells it apart from anything a foreign library might keep there, and only factors whose eval is this library's are looked at.
constexpr unsigned long long ROBUST_TAG = 0x726f627573745f6cULL;       // "robust_l"
struct RobustBlock { unsigned long long tag = ROBUST_TAG; int kind = 0; double c = 0; };
april_graph_factor_eval_t *xyt_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e);
april_graph_factor_eval_t *xytpos_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e);
bool is_library_common(const april_graph_factor_t *f) {
    return (f->type == APRIL_GRAPH_FACTOR_XYT_TYPE && f->nnodes == 2 && f->eval == xyt_eval) ||
           (f->type == APRIL_GRAPH_FACTOR_XYTPOS_TYPE && f->nnodes == 1 && f->eval == xytpos_eval);
}
RobustBlock *own_robust(const april_graph_factor_t *f) {
    if (!is_library_common(f)) return nullptr;
    void *p = f->u.common.impl;
    return (p && *(const unsigned long long *)p == ROBUST_TAG) ? (RobustBlock *)p : nullptr;
}

void eval_finish(april_graph_factor_t *f, april_graph_factor_eval_t *e) {
    e->length = 3;
    memcpy(e->W->data, f->u.common.W->data, 72);
    const double *w = e->W->data, *r = e->r;
    double X0 = w[0] * r[0] + w[1] * r[1] + w[2] * r[2];
    double X1 = w[3] * r[0] + w[4] * r[1] + w[5] * r[2];
    double X2 = w[6] * r[0] + w[7] * r[1] + w[8] * r[2];
    e->chi2 = r[0] * X0 + r[1] * X1 + r[2] * X2;
    if (const RobustBlock *rb = own_robust(f)) {      // IRLS: the plain r and J with W_eff = w(s) W, chi2 = rho(s)
        const double s = e->chi2, wt = asam::robust_weight(rb->kind, rb->c, s);
        for (int i = 0; i < 9; i++) e->W->data[i] = wt * e->W->data[i];
        e->chi2 = asam::robust_rho(rb->kind, rb->c, s);
    }
}

// ---- xyt factor ------------------------------------------------------------------------------------------
april_graph_factor_eval_t *xyt_eval_at(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e, bool at_state) {
    if (!e) e = eval_alloc(2);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    const double *pa = at_state ? ns[f->nodes[0]]->state : ns[f->nodes[0]]->l_point;
    const double *pb = at_state ? ns[f->nodes[1]]->state : ns[f->nodes[1]]->l_point;
    double ca = cos(pa[2]), sa = sin(pa[2]);
    double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    double zh0 = ca * dx + sa * dy, zh1 = -sa * dx + ca * dy, zh2 = pb[2] - pa[2];
    const double J0[9] = { -ca, -sa, -sa * dx + ca * dy, sa, -ca, -ca * dx - sa * dy, 0, 0, -1 };
    const double J1[9] = { ca, sa, 0, -sa, ca, 0, 0, 0, 1 };
    memcpy(e->jacobians[0]->data, J0, 72);
    memcpy(e->jacobians[1]->data, J1, 72);
    const double *z = f->u.common.z;
    e->r[0] = z[0] - zh0; e->r[1] = z[1] - zh1; e->r[2] = mod2pi_h(z[2] - zh2);
    eval_finish(f, e);
    return e;
}
april_graph_factor_eval_t *xyt_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return xyt_eval_at(f, g, e, false); }
april_graph_factor_eval_t *xyt_state_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return xyt_eval_at(f, g, e, true); }
// ---- attributes ----------------------------------------------------------------------------------------------
// The reference hangs a zhash of typed values off node->attr / factor->attr / graph->attr (april_graph.c:101-176).  This
// library keeps only what the `.graph` files of the path need: string values ("type" = "odom" / "scan" on the demo's
// factors, examples/aprilsam_demo.c:84-86), in insertion order.  The block starts with a tag so that an attr pointer
// set by the REFERENCE library (whose block starts with a heap pointer) is recognised as foreign and left alone.
constexpr unsigned long long ATTR_TAG = 0x617474725f616d64ULL;       // "attr_amd"
struct AmdAttr { unsigned long long tag = ATTR_TAG; std::vector<std::pair<std::string, std::string>> kv; };
AmdAttr *own_attr(const void *p) { return (p && *(const unsigned long long *)p == ATTR_TAG) ? (AmdAttr *)p : nullptr; }
void attr_free(void *p) { if (AmdAttr *a = own_attr(p)) delete a; }
void *attr_clone(const void *p) { const AmdAttr *a = own_attr(p); return a ? new AmdAttr(*a) : nullptr; }
int attr_put(void **slot, const char *key, const char *value) {
    if (!key || !value) return -1;
    if (*slot && !own_attr(*slot)) return -2;                        // attributes owned by another library
    if (!*slot) *slot = new AmdAttr();
    AmdAttr *a = (AmdAttr *)*slot;
    for (auto &kv : a->kv) if (kv.first == key) { kv.second = value; return 0; }
    a->kv.emplace_back(key, value);
    return 0;
}
const char *attr_get(const void *p, const char *key) {
    const AmdAttr *a = own_attr(p);
    if (!a || !key) return nullptr;
    for (auto &kv : a->kv) if (kv.first == key) return kv.second.c_str();
    return nullptr;
}

void factor_destroy(april_graph_factor_t *f) {
    delete own_robust(f);
    free(f->nodes); free(f->u.common.z); free(f->u.common.ztruth); free(f->u.common.W);
    attr_free(f->attr);
    free(f);
}
void robust_clone(const april_graph_factor_t *f, april_graph_factor_t *c) {
    if (const RobustBlock *rb = own_robust(f)) c->u.common.impl = new RobustBlock(*rb);
}
april_graph_factor_t *xyt_copy(april_graph_factor_t *f) {
    april_graph_factor_t *c = april_graph_factor_xyt_create(f->nodes[0], f->nodes[1], f->u.common.z, f->u.common.ztruth, f->u.common.W);
    c->attr = attr_clone(f->attr);            // the reference's copy keeps the attributes (the demo reads "type" from the copy)
    robust_clone(f, c);
    return c;
}

// ---- xytpos factor ----------------------------------------------------------------------------------------
april_graph_factor_eval_t *xytpos_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) {
    if (!e) e = eval_alloc(1);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    const double *pa = ns[f->nodes[0]]->state;                    // state, not l_point (april_graph_xytpos.c:83-85)
    double *J = e->jacobians[0]->data;
    J[0] = 1; J[4] = 1; J[8] = 1;
    const double *z = f->u.common.z;
    e->r[0] = z[0] - pa[0]; e->r[1] = z[1] - pa[1]; e->r[2] = mod2pi_h(z[2] - pa[2]);
    eval_finish(f, e);
    return e;
}
april_graph_factor_t *xytpos_copy(april_graph_factor_t *f) {
    april_graph_factor_t *c = april_graph_factor_xytpos_create(f->nodes[0], f->u.common.z, f->u.common.ztruth, f->u.common.W);
    c->attr = attr_clone(f->attr);
    robust_clone(f, c);
    return c;
}

// ---- xyt node ----------------------------------------------------------------------------------------------
void node_update(april_graph_node_t *n, double *d) {             // april_graph_xyt.c:302-314
    for (int i = 0; i < 3; i++) if (std::isnan(d[i])) return;
    for (int i = 0; i < 3; i++) n->state[i] = n->l_point[i] + d[i];
    for (int i = 0; i < 3; i++) n->delta_X[i] = d[i];
    n->state[2] = mod2pi_h(n->state[2]);
}
void node_relinearize(april_graph_node_t *n) { memcpy(n->l_point, n->state, 24); }    // april_graph_xyt.c:316-320
// ---- fixed nodes ----------------------------------------------------------------------
// The reference leaves node->impl unused (NULL) on its xyt nodes.  A node held constant points it at this block; the tag tells it apart from
// anything a foreign library might keep there, and only nodes whose destroy is this library's are looked at (the block is freed there).
constexpr unsigned long long FIXED_TAG = 0x66697865645f6e64ULL;        // "fixed_nd"
struct FixedBlock { unsigned long long tag = FIXED_TAG; };
std::atomic<bool> g_fixed_ever{ false };      // set by the first FixedBlock of the process (asam::fixed_ever)
FixedBlock *new_fixed() { g_fixed_ever.store(true, std::memory_order_relaxed); return new FixedBlock(); }
void node_destroy(april_graph_node_t *n);
FixedBlock *own_fixed(const april_graph_node_t *n) {
    if (n->type != APRIL_GRAPH_NODE_XYT_TYPE || n->destroy != node_destroy) return nullptr;
    void *p = n->impl;
    return (p && *(const unsigned long long *)p == FIXED_TAG) ? (FixedBlock *)p : nullptr;
}
void node_destroy(april_graph_node_t *n) {
    delete own_fixed(n);
    free(n->state); free(n->init); free(n->truth); free(n->l_point); free(n->delta_X); attr_free(n->attr); free(n);
}
april_graph_node_t *node_copy(april_graph_node_t *n) {
    april_graph_node_t *c = april_graph_node_xyt_create(n->state, n->init, n->truth);
    memcpy(c->l_point, n->l_point, 24); memcpy(c->delta_X, n->delta_X, 24);
    c->attr = attr_clone(n->attr);
    if (own_fixed(n)) c->impl = new_fixed();
    return c;
}

// ---- max-mixture factor -------------------------------------------------------------------
// u.max { factors, logw, nfactors } as the reference's union lays it out; the components are library xyt factors on the same (a, b)
april_graph_factor_eval_t *max_eval_at(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e, bool at_state) {
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    const double *pa = at_state ? ns[f->nodes[0]]->state : ns[f->nodes[0]]->l_point;
    const double *pb = at_state ? ns[f->nodes[1]]->state : ns[f->nodes[1]]->l_point;
    april_graph_factor_t *c = f->u.max.factors[asam::max_select(f, pa, pb)];
    return xyt_eval_at(c, g, e, at_state);
}
april_graph_factor_eval_t *max_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return max_eval_at(f, g, e, false); }
april_graph_factor_eval_t *max_state_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return max_eval_at(f, g, e, true); }
void max_destroy(april_graph_factor_t *f) {
    for (int i = 0; i < f->u.max.nfactors; i++) f->u.max.factors[i]->destroy(f->u.max.factors[i]);
    free(f->u.max.factors); free(f->u.max.logw); free(f->nodes);
    attr_free(f->attr);
    free(f);
}
april_graph_factor_t *max_make(april_graph_factor_t **components, const double *logw, int n) {
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(april_graph_factor_t));
    f->type = APRILSAM_AMD_FACTOR_MAX_TYPE;
    f->nnodes = 2;
    f->nodes = (int *)calloc(2, sizeof(int));
    f->nodes[0] = components[0]->nodes[0]; f->nodes[1] = components[0]->nodes[1];
    f->length = 3;
    f->u.max.factors = (april_graph_factor_t **)malloc(sizeof(april_graph_factor_t *) * (size_t)n);
    f->u.max.logw = (double *)malloc(sizeof(double) * (size_t)n);
    memcpy(f->u.max.factors, components, sizeof(april_graph_factor_t *) * (size_t)n);
    memcpy(f->u.max.logw, logw, sizeof(double) * (size_t)n);
    f->u.max.nfactors = n;
    return f;
}
april_graph_factor_t *max_copy(april_graph_factor_t *f) {
    const int n = f->u.max.nfactors;
    std::vector<april_graph_factor_t *> cs((size_t)n);
    for (int i = 0; i < n; i++) cs[i] = f->u.max.factors[i]->copy(f->u.max.factors[i]);
    april_graph_factor_t *c = max_make(cs.data(), f->u.max.logw, n);
    c->copy = f->copy; c->eval = f->eval; c->state_eval = f->state_eval; c->destroy = f->destroy;
    c->attr = attr_clone(f->attr);
    return c;
}

// ---- range / bearing / range-bearing factor -------------------------------------------------
// u.common as the reference lays it out: z holds m doubles, W is m x m (m = 1 or 2), ztruth stays NULL; the kind lives in a tagged block
// hung off u.common.impl (as a robust loss does on an xyt factor).
constexpr unsigned long long POLAR_TAG = 0x706f6c61725f616dULL;        // "polar_am"
struct PolarBlock { unsigned long long tag = POLAR_TAG; int kind = 0; };
april_graph_factor_eval_t *polar_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e);
PolarBlock *own_polar(const april_graph_factor_t *f) {
    if (f->type != APRILSAM_AMD_FACTOR_POLAR_TYPE || f->nnodes != 2 || f->eval != polar_eval) return nullptr;
    void *p = f->u.common.impl;
    return (p && *(const unsigned long long *)p == POLAR_TAG) ? (PolarBlock *)p : nullptr;
}
matd_t *matd_new(int nr, int nc, const double *data) {
    matd_t *m = (matd_t *)calloc(1, sizeof(matd_t) + (size_t)nr * nc * sizeof(double));
    m->nrows = nr; m->ncols = nc;
    if (data) memcpy(m->data, data, (size_t)nr * nc * sizeof(double));
    return m;
}
// april_graph_factor_eval_destroy frees `length` Jacobians (april_graph.c:38-43), and this factor has two nodes whatever its length: with
// m = 1 both Jacobians live in ONE block (the second is an interior pointer, freed with the first), with m = 2 in one block each
april_graph_factor_eval_t *polar_eval_alloc(int m) {
    april_graph_factor_eval_t *e = (april_graph_factor_eval_t *)calloc(1, sizeof(*e));
    e->jacobians = (matd_t **)calloc(3, sizeof(matd_t *));            // NULL-terminated
    const size_t one = sizeof(matd_t) + (size_t)m * 3 * sizeof(double);
    if (m == 1) {
        char *blk = (char *)calloc(2, one);
        e->jacobians[0] = (matd_t *)blk; e->jacobians[1] = (matd_t *)(blk + one);
    } else { e->jacobians[0] = (matd_t *)calloc(1, one); e->jacobians[1] = (matd_t *)calloc(1, one); }
    for (int i = 0; i < 2; i++) { e->jacobians[i]->nrows = m; e->jacobians[i]->ncols = 3; }
    e->r = (double *)calloc(m, sizeof(double));
    e->W = matd_new(m, m, nullptr);
    e->length = m;
    return e;
}
// the true m-row factor: r = z - h(q), J = G J_xyt (rows 0, 1 of the xyt Jacobians), W, chi2 = r' W r.  rho^2 == 0: J = 0
april_graph_factor_eval_t *polar_eval_at(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e, bool at_state) {
    const PolarBlock *pb_ = own_polar(f);
    if (!pb_) return nullptr;
    const int kind = pb_->kind, m = asam::polar_rows(kind);
    if (!e) e = polar_eval_alloc(m);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    const double *pa = at_state ? ns[f->nodes[0]]->state : ns[f->nodes[0]]->l_point;
    const double *pb = at_state ? ns[f->nodes[1]]->state : ns[f->nodes[1]]->l_point;
    const double ca = cos(pa[2]), sa = sin(pa[2]);
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    const double q0 = ca * dx + sa * dy, q1 = -sa * dx + ca * dy;
    const double Jx[2][6] = { { -ca, -sa, -sa * dx + ca * dy, sa, -ca, -ca * dx - sa * dy }, { ca, sa, 0, -sa, ca, 0 } };
    double G[4] = { 0, 0, 0, 0 };
    (void)asam::polar_G(kind, q0, q1, G);
    for (int n = 0; n < 2; n++)
        for (int i = 0; i < m; i++)
            for (int j = 0; j < 3; j++) e->jacobians[n]->data[i * 3 + j] = G[2 * i] * Jx[n][j] + G[2 * i + 1] * Jx[n][3 + j];
    asam::polar_residual(kind, f->u.common.z, q0, q1, e->r);
    e->length = m;
    memcpy(e->W->data, f->u.common.W->data, sizeof(double) * (size_t)m * m);
    e->chi2 = asam::polar_cost(kind, f->u.common.z, f->u.common.W->data, q0, q1);
    return e;
}
april_graph_factor_eval_t *polar_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return polar_eval_at(f, g, e, false); }
april_graph_factor_eval_t *polar_state_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return polar_eval_at(f, g, e, true); }
void polar_destroy(april_graph_factor_t *f) {
    delete own_polar(f);
    free(f->nodes); free(f->u.common.z); free(f->u.common.ztruth); free(f->u.common.W);
    attr_free(f->attr);
    free(f);
}
april_graph_factor_t *polar_make(int kind, int a, int b, const double *z, const double *W) {
    const int m = asam::polar_rows(kind);
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(april_graph_factor_t));
    f->type = APRILSAM_AMD_FACTOR_POLAR_TYPE;
    f->nnodes = 2;
    f->nodes = (int *)calloc(2, sizeof(int));
    f->nodes[0] = a; f->nodes[1] = b;
    f->length = m;
    f->u.common.z = (double *)malloc(sizeof(double) * (size_t)m);
    memcpy(f->u.common.z, z, sizeof(double) * (size_t)m);
    f->u.common.W = matd_new(m, m, W);
    PolarBlock *blk = new PolarBlock(); blk->kind = kind;
    f->u.common.impl = blk;
    return f;
}
april_graph_factor_t *polar_copy(april_graph_factor_t *f) {
    const PolarBlock *pb_ = own_polar(f);
    if (!pb_) return nullptr;
    april_graph_factor_t *c = polar_make(pb_->kind, f->nodes[0], f->nodes[1], f->u.common.z, f->u.common.W->data);
    c->copy = f->copy; c->eval = f->eval; c->state_eval = f->state_eval; c->destroy = f->destroy;
    c->attr = attr_clone(f->attr);
    return c;
}

// ---- dense Gaussian factor on k nodes, information form --------------------------------------
// u.common as the reference lays it out: z holds xbar (3 k) then eta (3 k), W is Lambda (3 k x 3 k), ztruth stays NULL; the square-root
// form the host evaluation returns lives in a tagged block hung off u.common.impl, with a copy of the eta and Lambda it was made from
// (z and W may be edited in place: gaussian_refresh factorises again).
constexpr unsigned long long GAUSSIAN_TAG = 0x67617573735f616dULL;     // "gauss_am"
struct GaussianBlock {
    unsigned long long tag = GAUSSIAN_TAG; int k = 0, rank = 0; bool ok = false; double c0 = 0;
    std::vector<double> R, d, snap;      // R: rank x 3k row-major (R'R = Lambda), d: rank (R'd = eta), snap: eta (3k) + Lambda (9 k^2) as factorised
};
std::atomic<bool> g_gaussian_ever{ false };
april_graph_factor_eval_t *gaussian_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e);
GaussianBlock *own_gaussian(const april_graph_factor_t *f) {
    if (f->type != APRILSAM_AMD_FACTOR_GAUSSIAN_TYPE || f->eval != gaussian_eval) return nullptr;
    void *p = f->u.common.impl;
    GaussianBlock *b = (p && *(const unsigned long long *)p == GAUSSIAN_TAG) ? (GaussianBlock *)p : nullptr;
    return (b && f->nnodes == b->k && f->nodes && f->u.common.z && f->u.common.W) ? b : nullptr;
}
// Diagonally pivoted Cholesky of the n x n matrix L (row-major, bitwise symmetric), LAPACK dpstrf's default stop: the largest remaining
// diagonal <= n eps max diag.  R (rank x n, columns in the ORIGINAL order) with R'R = L; d with R'd = eta from the triangular solve in pivot
// order.  false: L is not finite, not symmetric or not positive semi-definite (a remaining diagonal below -10 times the stop bound)
bool gaussian_factorise(int n, const double *eta, const double *L, int *rank_out, std::vector<double> &R, std::vector<double> &d, double *c0) {
    for (int i = 0; i < n; i++) {
        if (!std::isfinite(eta[i])) return false;
        for (int j = 0; j < n; j++) {
            if (!std::isfinite(L[(size_t)i * n + j])) return false;
            if (memcmp(&L[(size_t)i * n + j], &L[(size_t)j * n + i], 8) != 0) return false;
        }
    }
    std::vector<double> A(L, L + (size_t)n * n), Rp((size_t)n * n, 0.0);
    std::vector<int> piv((size_t)n);
    for (int i = 0; i < n; i++) piv[i] = i;
    double amax = 0;
    for (int i = 0; i < n; i++) { if (A[(size_t)i * n + i] < 0) return false; amax = std::max(amax, A[(size_t)i * n + i]); }
    const double tol = (double)n * 2.220446049250313e-16 * amax;
    int rank = 0;
    for (int j = 0; j < n; j++) {
        int p = j;
        for (int i = j + 1; i < n; i++) if (A[(size_t)i * n + i] > A[(size_t)p * n + p]) p = i;      // (the first of equal candidates)
        if (!(A[(size_t)p * n + p] > tol)) break;
        if (p != j) {                  // symmetric interchange of the remainder, and of the columns of the rows of R made so far
            for (int i = 0; i < n; i++) std::swap(A[(size_t)i * n + j], A[(size_t)i * n + p]);
            for (int i = 0; i < n; i++) std::swap(A[(size_t)j * n + i], A[(size_t)p * n + i]);
            for (int l = 0; l < j; l++) std::swap(Rp[(size_t)l * n + j], Rp[(size_t)l * n + p]);
            std::swap(piv[j], piv[p]);
        }
        const double rjj = sqrt(A[(size_t)j * n + j]);
        Rp[(size_t)j * n + j] = rjj;
        for (int i = j + 1; i < n; i++) Rp[(size_t)j * n + i] = A[(size_t)j * n + i] / rjj;
        for (int i = j + 1; i < n; i++)
            for (int l = j + 1; l < n; l++) A[(size_t)i * n + l] -= Rp[(size_t)j * n + i] * Rp[(size_t)j * n + l];
        rank = j + 1;
    }
    for (int i = rank; i < n; i++) if (A[(size_t)i * n + i] < -10.0 * tol) return false;
    if (amax == 0)                     // (a zero diagonal: positive semi-definite only as the zero matrix)
        for (size_t i = 0; i < (size_t)n * n; i++) if (L[i] != 0) return false;
    R.assign((size_t)rank * n, 0.0); d.assign((size_t)rank, 0.0);
    for (int l = 0; l < rank; l++)
        for (int c = 0; c < n; c++) R[(size_t)l * n + piv[c]] = Rp[(size_t)l * n + c];
    double cc = 0;
    for (int l = 0; l < rank; l++) {   // R11' d = (P' eta)[0:rank], forward
        double acc = eta[piv[l]];
        for (int m = 0; m < l; m++) acc -= Rp[(size_t)m * n + l] * d[m];
        d[l] = acc / Rp[(size_t)l * n + l];
        cc += d[l] * d[l];
    }
    *rank_out = rank; *c0 = cc;
    return true;
}
// the block against the object: factorised again when eta or Lambda were edited in place.  false: they are not admissible (any more)
bool gaussian_refresh(const april_graph_factor_t *f, GaussianBlock *b) {
    const int n = 3 * b->k;
    if ((int)f->u.common.W->nrows != n || (int)f->u.common.W->ncols != n) { b->ok = false; b->snap.clear(); return false; }
    const double *eta = f->u.common.z + n, *L = f->u.common.W->data;
    const size_t nl = (size_t)n * n;
    if (b->snap.size() == n + nl && memcmp(b->snap.data(), eta, (size_t)8 * n) == 0 && memcmp(b->snap.data() + n, L, 8 * nl) == 0) return b->ok;
    b->snap.assign(eta, eta + n); b->snap.insert(b->snap.end(), L, L + nl);
    b->ok = gaussian_factorise(n, eta, L, &b->rank, b->R, b->d, &b->c0);
    if (!b->ok) { b->rank = 0; b->R.clear(); b->d.clear(); b->c0 = 0; }
    return b->ok;
}
// april_graph_factor_eval_destroy frees the Jacobians [0, min(length, k)) and r (april_graph.c:38-46): those Jacobians are blocks of their
// own, the others live behind r in r's block
april_graph_factor_eval_t *gaussian_eval_alloc(int k, int L) {
    april_graph_factor_eval_t *e = (april_graph_factor_eval_t *)calloc(1, sizeof(*e));
    e->jacobians = (matd_t **)calloc((size_t)k + 1, sizeof(matd_t *));            // NULL-terminated
    const size_t one = sizeof(matd_t) + (size_t)L * 3 * sizeof(double), rlen = (size_t)std::max(L, 1) * sizeof(double);
    const int nsep = std::min(L, k);
    for (int i = 0; i < nsep; i++) e->jacobians[i] = (matd_t *)calloc(1, one);
    char *blk = (char *)calloc(1, rlen + (size_t)(k - nsep) * one);
    e->r = (double *)blk;
    for (int i = nsep; i < k; i++) e->jacobians[i] = (matd_t *)(blk + rlen + (size_t)(i - nsep) * one);
    for (int i = 0; i < k; i++) { e->jacobians[i]->nrows = (unsigned)L; e->jacobians[i]->ncols = 3; }
    e->W = matd_new(L, L, nullptr);
    e->length = L;
    return e;
}
april_graph_factor_eval_t *gaussian_eval_at(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e, bool at_state) {
    GaussianBlock *b = own_gaussian(f);
    if (!b || !gaussian_refresh(f, b)) return nullptr;
    const int k = b->k, n = 3 * k, L = b->rank;
    if (e && e->length != L) { april_graph_factor_eval_destroy(e); e = nullptr; }      // (the rank changed with an edit)
    if (!e) e = gaussian_eval_alloc(k, L);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    std::vector<double> delta((size_t)n);
    for (int i = 0; i < k; i++) {
        const double *p = at_state ? ns[f->nodes[i]]->state : ns[f->nodes[i]]->l_point, *xb = f->u.common.z + 3 * i;
        delta[3 * i] = p[0] - xb[0]; delta[3 * i + 1] = p[1] - xb[1]; delta[3 * i + 2] = mod2pi_h(p[2] - xb[2]);
    }
    double chi2 = 0;
    for (int l = 0; l < L; l++) {
        double acc = 0;
        for (int c = 0; c < n; c++) acc += b->R[(size_t)l * n + c] * delta[c];
        e->r[l] = b->d[l] - acc;
        chi2 += e->r[l] * e->r[l];
        for (int i = 0; i < k; i++)
            for (int c = 0; c < 3; c++) e->jacobians[i]->data[l * 3 + c] = b->R[(size_t)l * n + 3 * i + c];
        for (int m = 0; m < L; m++) e->W->data[(size_t)l * L + m] = l == m ? 1.0 : 0.0;
    }
    e->length = L; e->chi2 = chi2;
    return e;
}
april_graph_factor_eval_t *gaussian_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return gaussian_eval_at(f, g, e, false); }
april_graph_factor_eval_t *gaussian_state_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return gaussian_eval_at(f, g, e, true); }
void gaussian_destroy(april_graph_factor_t *f) {
    delete own_gaussian(f);
    free(f->nodes); free(f->u.common.z); free(f->u.common.ztruth); free(f->u.common.W);
    attr_free(f->attr);
    free(f);
}
april_graph_factor_t *gaussian_copy(april_graph_factor_t *f);
// nullptr when eta / Lambda are refused (nothing is owned then)
april_graph_factor_t *gaussian_make(int k, const int *nodes, const double *xbar_eta, const double *Lambda) {
    const int n = 3 * k;
    GaussianBlock *blk = new GaussianBlock(); blk->k = k;
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(april_graph_factor_t));
    f->type = APRILSAM_AMD_FACTOR_GAUSSIAN_TYPE;
    f->nnodes = k;
    f->nodes = (int *)calloc((size_t)k, sizeof(int));
    memcpy(f->nodes, nodes, sizeof(int) * (size_t)k);
    f->u.common.z = (double *)malloc(sizeof(double) * (size_t)2 * n);
    memcpy(f->u.common.z, xbar_eta, sizeof(double) * (size_t)2 * n);
    f->u.common.W = matd_new(n, n, Lambda);
    f->u.common.impl = blk;
    f->copy = gaussian_copy; f->eval = gaussian_eval; f->state_eval = gaussian_state_eval; f->destroy = gaussian_destroy;
    if (!gaussian_refresh(f, blk)) { gaussian_destroy(f); return nullptr; }
    f->length = blk->rank;
    g_gaussian_ever.store(true, std::memory_order_relaxed);
    return f;
}
april_graph_factor_t *gaussian_copy(april_graph_factor_t *f) {
    if (!own_gaussian(f)) return nullptr;
    april_graph_factor_t *c = gaussian_make(f->nnodes, f->nodes, f->u.common.z, f->u.common.W->data);
    if (c) c->attr = attr_clone(f->attr);
    return c;
}

}  // namespace

namespace asam {

bool gaussian_of(const april_graph_factor_t *f, int *k, double *c0, bool *ok) {
    GaussianBlock *b = own_gaussian(f);
    if (!b) return false;
    const bool good = gaussian_refresh(f, b);
    if (k) *k = b->k;
    if (c0) *c0 = b->c0;
    if (ok) *ok = good;
    return true;
}
bool gaussian_ever() { return g_gaussian_ever.load(std::memory_order_relaxed); }

bool is_native_max(const april_graph_factor_t *f) { return f->type == APRILSAM_AMD_FACTOR_MAX_TYPE && f->eval == max_eval; }

double max_det3(const double *w) {
    return w[0] * (w[4] * w[8] - w[5] * w[7]) - w[1] * (w[3] * w[8] - w[5] * w[6]) + w[2] * (w[3] * w[7] - w[4] * w[6]);
}
// c_i = -2 logw_i - ln det W_i: the part of a component's score that does not depend on the point
double max_const(const april_graph_factor_t *f, int i) {
    return -2.0 * f->u.max.logw[i] - log(max_det3(f->u.max.factors[i]->u.common.W->data));
}

bool max_check(const april_graph_factor_t *f, char *why, int cap) {
    const int n = f->u.max.nfactors;
    if (n < 1 || n > MAX_MIX_K || !f->u.max.factors || !f->u.max.logw) { snprintf(why, cap, "%d components (1 to %d are supported)", n, MAX_MIX_K); return false; }
    for (int i = 0; i < n; i++) {
        const april_graph_factor_t *c = f->u.max.factors[i];
        if (!c || c->type != APRIL_GRAPH_FACTOR_XYT_TYPE || c->nnodes != 2 || c->eval != xyt_eval || !c->u.common.z || !c->u.common.W) {
            snprintf(why, cap, "component %d is not an xyt factor of this library (april_graph_factor_xyt_create)", i); return false;
        }
        if (own_robust(c)) { snprintf(why, cap, "component %d carries a robust loss (DESIGN.md section 15: not supported on max factors)", i); return false; }
        if (c->nodes[0] != f->nodes[0] || c->nodes[1] != f->nodes[1]) {
            snprintf(why, cap, "component %d connects (%d, %d), the factor (%d, %d)", i, c->nodes[0], c->nodes[1], f->nodes[0], f->nodes[1]); return false;
        }
        const double *w = c->u.common.W->data;
        if (w[1] != w[3] || w[2] != w[6] || w[5] != w[7]) { snprintf(why, cap, "component %d: W is not symmetric", i); return false; }
        if (!(max_det3(w) > 0)) { snprintf(why, cap, "component %d: det W = %g is not positive", i, max_det3(w)); return false; }
        if (!std::isfinite(f->u.max.logw[i])) { snprintf(why, cap, "component %d: logw = %g is not finite", i, f->u.max.logw[i]); return false; }
    }
    return true;
}

// the selection rule of DESIGN.md section 12 at poses pa, pb: the score r^T W r (eval_finish's association) + c_i, lowest index on a tie or NaN
int max_select(const april_graph_factor_t *f, const double *pa, const double *pb) {
    const double ca = cos(pa[2]), sa = sin(pa[2]);
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    const double zh0 = ca * dx + sa * dy, zh1 = -sa * dx + ca * dy, zh2 = pb[2] - pa[2];
    int best = 0; double sbest = 0;
    for (int i = 0; i < f->u.max.nfactors; i++) {
        const april_graph_factor_t *c = f->u.max.factors[i];
        const double *z = c->u.common.z, *w = c->u.common.W->data;
        const double r[3] = { z[0] - zh0, z[1] - zh1, mod2pi_h(z[2] - zh2) };
        const double X0 = w[0] * r[0] + w[1] * r[1] + w[2] * r[2];
        const double X1 = w[3] * r[0] + w[4] * r[1] + w[5] * r[2];
        const double X2 = w[6] * r[0] + w[7] * r[1] + w[8] * r[2];
        const double s = (r[0] * X0 + r[1] * X1 + r[2] * X2) + max_const(f, i);
        if (i == 0) sbest = s;
        else if (s < sbest) { best = i; sbest = s; }
    }
    return best;
}

// s = r^T W r of an xyt (pb given) or xytpos factor with measurement z at pa / pb, in eval_finish's association
double robust_host_s(const double *z, const double *w, const double *pa, const double *pb) {
    double r[3];
    if (pb) {
        const double ca = cos(pa[2]), sa = sin(pa[2]);
        const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
        const double zh0 = ca * dx + sa * dy, zh1 = -sa * dx + ca * dy, zh2 = pb[2] - pa[2];
        r[0] = z[0] - zh0; r[1] = z[1] - zh1; r[2] = mod2pi_h(z[2] - zh2);
    } else {
        r[0] = z[0] - pa[0]; r[1] = z[1] - pa[1]; r[2] = mod2pi_h(z[2] - pa[2]);
    }
    const double X0 = w[0] * r[0] + w[1] * r[1] + w[2] * r[2];
    const double X1 = w[3] * r[0] + w[4] * r[1] + w[5] * r[2];
    const double X2 = w[6] * r[0] + w[7] * r[1] + w[8] * r[2];
    return r[0] * X0 + r[1] * X1 + r[2] * X2;
}

bool polar_of(const april_graph_factor_t *f, int *kind) {
    const PolarBlock *pb = own_polar(f);
    if (!pb || !f->u.common.z || !f->u.common.W) return false;
    *kind = pb->kind;
    return true;
}
bool node_fixed(const april_graph_node_t *n) { return n && own_fixed(n) != nullptr; }
bool fixed_ever() { return g_fixed_ever.load(std::memory_order_relaxed); }
bool plain_common_factor(const april_graph_factor_t *f) { return is_library_common(f) && f->u.common.W && f->u.common.z; }
bool robust_of(const april_graph_factor_t *f, int *kind, double *c) {
    const RobustBlock *rb = own_robust(f);
    if (!rb) return false;
    *kind = rb->kind; *c = rb->c;
    return true;
}

}  // namespace asam

extern "C" {

int aprilsam_amd_factor_set_robust(april_graph_factor_t *f, int kind, double c) {
    const char *who = "aprilsam_amd_factor_set_robust: ";
    if (!f) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "null factor"); return asam::ERR_BAD_GRAPH; }
    if (!is_library_common(f) || !f->u.common.W || !f->u.common.z) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "not an xyt / xytpos factor of this library (max factors and foreign factors carry no loss)");
        return asam::ERR_UNSUPPORTED;
    }
    if (f->u.common.impl && !own_robust(f)) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "u.common.impl is in use by another library");
        return asam::ERR_UNSUPPORTED;
    }
    if (kind < APRILSAM_AMD_ROBUST_NONE || kind > APRILSAM_AMD_ROBUST_DCS) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "kind " + std::to_string(kind) + " out of range (0 to 3)");
        return asam::ERR_BAD_GRAPH;
    }
    if (kind == APRILSAM_AMD_ROBUST_NONE) { delete own_robust(f); f->u.common.impl = nullptr; return 0; }
    if (!std::isfinite(c) || !(c > 0)) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "c = " + std::to_string(c) + " must be finite and > 0");
        return asam::ERR_BAD_GRAPH;
    }
    if (!asam::robust_spd(f->u.common.W->data)) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "W is not symmetric positive definite");
        return asam::ERR_UNSUPPORTED;
    }
    RobustBlock *rb = own_robust(f);
    if (!rb) { rb = new RobustBlock(); f->u.common.impl = rb; }
    rb->kind = kind; rb->c = c;
    return 0;
}

int aprilsam_amd_node_set_fixed(april_graph_node_t *node, int fixed) {
    const char *who = "aprilsam_amd_node_set_fixed: ";
    if (!node) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "null node"); return asam::ERR_BAD_GRAPH; }
    if (fixed != 0 && fixed != 1) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "fixed = " + std::to_string(fixed) + " (0 or 1)");
        return asam::ERR_BAD_GRAPH;
    }
    if (node->type != APRIL_GRAPH_NODE_XYT_TYPE || node->destroy != node_destroy) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "not an xyt node of this library");
        return asam::ERR_UNSUPPORTED;
    }
    if (node->impl && !own_fixed(node)) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "node->impl is in use by another library");
        return asam::ERR_UNSUPPORTED;
    }
    if (!fixed) { delete own_fixed(node); node->impl = nullptr; return 0; }
    if (!node->impl) node->impl = new_fixed();
    return 0;
}

int aprilsam_amd_node_get_fixed(const april_graph_node_t *node) { return asam::node_fixed(node) ? 1 : 0; }

int aprilsam_amd_factor_get_robust(const april_graph_factor_t *f, int *kind, double *c) {
    int k = APRILSAM_AMD_ROBUST_NONE; double cv = 0;
    if (f) (void)asam::robust_of(f, &k, &cv);
    if (kind) *kind = k;
    if (c) *c = cv;
    return 0;
}

april_graph_factor_t *aprilsam_amd_factor_max_create(april_graph_factor_t **components, const double *logw, int n) {
    if (!components || !logw || n < 1 || n > asam::MAX_MIX_K) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, "aprilsam_amd_factor_max_create: " + std::to_string(n) + " components (1 to " + std::to_string(asam::MAX_MIX_K) +
                             " are supported) or a null argument");
        return nullptr;
    }
    for (int i = 0; i < n; i++)
        if (!components[i] || components[i]->nnodes != 2 || !components[i]->nodes) {
            asam::set_last_error(asam::ERR_UNSUPPORTED, "aprilsam_amd_factor_max_create: component " + std::to_string(i) + " is not a binary factor");
            return nullptr;
        }
    april_graph_factor_t *f = max_make(components, logw, n);
    char why[256];
    if (!asam::max_check(f, why, sizeof why)) {     // (the caller keeps its components)
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string("aprilsam_amd_factor_max_create: ") + why);
        free(f->u.max.factors); free(f->u.max.logw); free(f->nodes); free(f);
        return nullptr;
    }
    f->copy = max_copy; f->eval = max_eval; f->state_eval = max_state_eval; f->destroy = max_destroy;
    return f;
}

april_graph_factor_t *aprilsam_amd_factor_polar_create(int kind, int a, int b, const double *z, const double *W) {
    const char *who = "aprilsam_amd_factor_polar_create: ";
    if (kind < APRILSAM_AMD_POLAR_RANGE || kind > APRILSAM_AMD_POLAR_RANGE_BEARING || !z || !W) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "kind " + std::to_string(kind) + " out of range (1 to 3) or a null argument");
        return nullptr;
    }
    if (a == b) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "nodes (" + std::to_string(a) + ", " + std::to_string(b) + "): two different nodes are needed");
        return nullptr;
    }
    const int m = asam::polar_rows(kind);
    for (int i = 0; i < m; i++)
        if (!std::isfinite(z[i])) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "z is not finite"); return nullptr; }
    if (!asam::polar_spd(kind, W)) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "W must be finite, symmetric (mirror entries bitwise equal) and positive definite");
        return nullptr;
    }
    april_graph_factor_t *f = polar_make(kind, a, b, z, W);
    f->copy = polar_copy; f->eval = polar_eval; f->state_eval = polar_state_eval; f->destroy = polar_destroy;
    return f;
}

int aprilsam_amd_factor_get_polar(const april_graph_factor_t *f, int *kind) {
    int k = 0;
    if (f) (void)asam::polar_of(f, &k);
    if (kind) *kind = k;
    return 0;
}

april_graph_factor_t *aprilsam_amd_factor_gaussian_create(int k, const int *nodes, const double *xbar, const double *eta, const double *Lambda) {
    const char *who = "aprilsam_amd_factor_gaussian_create: ";
    if (!nodes || !xbar || !eta || !Lambda || k < 1) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "k = " + std::to_string(k) + " (at least 1) or a null argument");
        return nullptr;
    }
    if (k > APRILSAM_AMD_GAUSSIAN_MAX_NODES) {
        asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "k = " + std::to_string(k) + " nodes (1 to " + std::to_string(APRILSAM_AMD_GAUSSIAN_MAX_NODES) +
                             " are supported: the clique limit of factors with more than two nodes)");
        return nullptr;
    }
    for (int i = 0; i < k; i++)
        for (int j = 0; j < i; j++)
            if (nodes[i] == nodes[j]) {
                asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "node " + std::to_string(nodes[i]) + " is named twice: the node ids must be distinct");
                return nullptr;
            }
    std::vector<double> ze((size_t)6 * k);
    for (int i = 0; i < 3 * k; i++) {
        if (!std::isfinite(xbar[i]) || !std::isfinite(eta[i])) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "xbar and eta must be finite"); return nullptr; }
        ze[i] = xbar[i]; ze[(size_t)3 * k + i] = eta[i];
    }
    april_graph_factor_t *f = gaussian_make(k, nodes, ze.data(), Lambda);
    if (!f) asam::set_last_error(asam::ERR_UNSUPPORTED, std::string(who) + "Lambda must be finite, symmetric (mirror entries bitwise equal) and positive semi-definite");
    return f;
}

int aprilsam_amd_factor_get_gaussian(const april_graph_factor_t *f, int *k) {
    int kk = 0;
    if (f) (void)asam::gaussian_of(f, &kk, nullptr, nullptr);
    if (k) *k = kk;
    return 0;
}

int aprilsam_amd_debug_polar_slot(int kind, const double *pa, const double *pb, const double *z, const double *W, double *z_eff3, double *W_eff9) {
    if (kind < APRILSAM_AMD_POLAR_RANGE || kind > APRILSAM_AMD_POLAR_RANGE_BEARING || !pa || !pb || !z || !W || !z_eff3 || !W_eff9) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, "aprilsam_amd_debug_polar_slot: kind out of range (1 to 3) or a null argument");
        return asam::ERR_BAD_GRAPH;
    }
    asam::polar_host_slot(kind, z, W, pa, pb, z_eff3, W_eff9);
    return 0;
}

int aprilsam_amd_debug_polar_gate(int kind, const double *pa, const double *pb, const double *z, const double *W, const double *cov36, double *d2, double *S4) {
    if (kind < APRILSAM_AMD_POLAR_RANGE || kind > APRILSAM_AMD_POLAR_RANGE_BEARING || !pa || !pb || !z || !W || !cov36 || !d2 || !S4) {
        asam::set_last_error(asam::ERR_BAD_GRAPH, "aprilsam_amd_debug_polar_gate: kind out of range (1 to 3) or a null argument");
        return asam::ERR_BAD_GRAPH;
    }
    double S[4] = { 0.0, 0.0, 0.0, 0.0 };
    const bool ok = asam::polar_gate(kind, z, W, pa, pb, cov36, d2, S);
    for (int i = 0; i < 4; i++) S4[i] = S[i];
    return ok ? 0 : 1;
}

april_graph_t *april_graph_create(void) {
    april_graph_t *g = (april_graph_t *)calloc(1, sizeof(april_graph_t));
    g->factors = zarray_new(sizeof(april_graph_factor_t *));
    g->nodes = zarray_new(sizeof(april_graph_node_t *));
    return g;
}

void april_graph_destroy(april_graph_t *g) {
    if (!g) return;
    asam::drop_graph_pack(g);
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < g->nodes->size; i++) ns[i]->destroy(ns[i]);
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    for (int i = 0; i < g->factors->size; i++) fs[i]->destroy(fs[i]);
    free(g->nodes->data); free(g->nodes);
    free(g->factors->data); free(g->factors);
    attr_free(g->attr);
    free(g);
}

// the graph edit.  Everything is validated before anything is touched
int aprilsam_amd_graph_remove_nodes(april_graph_t *g, int m, const int *remove, int *new_index) {
    const char *who = "aprilsam_amd_graph_remove_nodes: ";
    if (!g || !g->nodes || !g->factors || m < 0 || (m > 0 && !remove)) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "null argument or negative count"); return asam::ERR_BAD_GRAPH; }
    const int N = g->nodes->size, F = g->factors->size;
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    std::vector<int> idx((size_t)N, 0);               // 0: kept, -1: removed; the new index afterwards
    for (int i = 0; i < m; i++) {
        if (remove[i] < 0 || remove[i] >= N) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "node " + std::to_string(remove[i]) + " out of range (" + std::to_string(N) + " nodes)"); return asam::ERR_BAD_GRAPH; }
        if (idx[remove[i]] < 0) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "node " + std::to_string(remove[i]) + " is listed twice"); return asam::ERR_BAD_GRAPH; }
        idx[remove[i]] = -1;
    }
    auto nodes_ok = [&](const april_graph_factor_t *f) {
        if (!f || f->nnodes < 0 || (f->nnodes > 0 && !f->nodes)) return false;
        for (int k = 0; k < f->nnodes; k++) if (f->nodes[k] < 0 || f->nodes[k] >= N) return false;
        return true;
    };
    for (int i = 0; i < F; i++) {
        bool ok = nodes_ok(fs[i]);
        if (ok && asam::is_native_max(fs[i]))
            for (int j = 0; j < fs[i]->u.max.nfactors && ok; j++) ok = nodes_ok(fs[i]->u.max.factors[j]);
        if (!ok) { asam::set_last_error(asam::ERR_BAD_GRAPH, std::string(who) + "factor " + std::to_string(i) + " names a node outside the graph"); return asam::ERR_BAD_GRAPH; }
    }
    for (int i = 0, k = 0; i < N; i++) if (idx[i] == 0) idx[i] = k++;
    if (new_index) memcpy(new_index, idx.data(), sizeof(int) * (size_t)N);
    if (m == 0) return 0;
    asam::drop_graph_pack(g);                         // (the device copy describes the graph before the edit)
    int nf = 0;
    for (int i = 0; i < F; i++) {
        april_graph_factor_t *f = fs[i];
        bool gone = false;                            // (a max factor is judged by its own nodes)
        for (int k = 0; k < f->nnodes; k++) gone = gone || idx[f->nodes[k]] < 0;
        if (gone) { f->destroy(f); continue; }
        for (int k = 0; k < f->nnodes; k++) f->nodes[k] = idx[f->nodes[k]];
        if (asam::is_native_max(f))
            for (int j = 0; j < f->u.max.nfactors; j++) {
                april_graph_factor_t *cf = f->u.max.factors[j];
                for (int k = 0; k < cf->nnodes; k++) cf->nodes[k] = idx[cf->nodes[k]] < 0 ? cf->nodes[k] : idx[cf->nodes[k]];
            }
        fs[nf++] = f;
    }
    g->factors->size = nf;
    int nn = 0;
    for (int i = 0; i < N; i++) {
        if (idx[i] < 0) { ns[i]->destroy(ns[i]); continue; }
        ns[nn++] = ns[i];
    }
    g->nodes->size = nn;
    return 0;
}

april_graph_node_t *april_graph_node_xyt_create(const double *state, const double *init, const double *truth) {
    april_graph_node_t *n = (april_graph_node_t *)calloc(1, sizeof(april_graph_node_t));
    n->type = APRIL_GRAPH_NODE_XYT_TYPE;
    n->length = 3;
    n->state = dup3(state); n->init = dup3(init); n->truth = dup3(truth);
    n->l_point = dup3(state);
    n->delta_X = (double *)calloc(3, sizeof(double));
    n->update = node_update; n->copy = node_copy; n->relinearize = node_relinearize; n->destroy = node_destroy;
    return n;
}

april_graph_factor_t *april_graph_factor_xyt_create(int a, int b, const double *z, const double *ztruth, const matd_t *W) {
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(april_graph_factor_t));
    f->type = APRIL_GRAPH_FACTOR_XYT_TYPE;
    f->nnodes = 2;
    f->nodes = (int *)calloc(2, sizeof(int));
    f->nodes[0] = a; f->nodes[1] = b;
    f->length = 3;
    f->copy = xyt_copy; f->eval = xyt_eval; f->state_eval = xyt_state_eval; f->destroy = factor_destroy;
    f->u.common.z = dup3(z); f->u.common.ztruth = dup3(ztruth); f->u.common.W = matd33(W ? W->data : nullptr);
    return f;
}

april_graph_factor_t *april_graph_factor_xytpos_create(int a, double *z, double *ztruth, matd_t *W) {
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(april_graph_factor_t));
    f->type = APRIL_GRAPH_FACTOR_XYTPOS_TYPE;
    f->nnodes = 1;
    f->nodes = (int *)calloc(1, sizeof(int));
    f->nodes[0] = a;
    f->length = 3;
    f->copy = xytpos_copy; f->eval = xytpos_eval; f->destroy = factor_destroy;
    f->u.common.z = dup3(z); f->u.common.ztruth = dup3(ztruth); f->u.common.W = matd33(W ? W->data : nullptr);
    return f;
}

void april_graph_factor_eval_destroy(april_graph_factor_eval_t *e) {      // april_graph.c:33-49
    if (!e) return;
    for (int i = 0; i < e->length; i++) { if (!e->jacobians[i]) break; free(e->jacobians[i]); }
    free(e->jacobians); free(e->r); free(e->W); free(e);
}

int april_graph_dof(april_graph_t *g) {                                  // april_graph.c:57-77
    int fd = 0, sd = 0;
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    for (int i = 0; i < g->nodes->size; i++) sd += ns[i]->length;
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    for (int i = 0; i < g->factors->size; i++) fd += fs[i]->length;
    return fd - sd;
}

void aprilsam_amd_graph_add_node(april_graph_t *g, april_graph_node_t *n) { zarray_append(g->nodes, &n); }
void aprilsam_amd_graph_add_factor(april_graph_t *g, april_graph_factor_t *f) { zarray_append(g->factors, &f); }

int aprilsam_amd_attr_put_string(void **attr_slot, const char *key, const char *value) { return attr_slot ? attr_put(attr_slot, key, value) : -1; }
const char *aprilsam_amd_attr_get_string(const void *attr, const char *key) { return attr_get(attr, key); }
int aprilsam_amd_attr_count(const void *attr) { const AmdAttr *a = own_attr(attr); return a ? (int)a->kv.size() : 0; }
int aprilsam_amd_attr_item(const void *attr, int i, const char **key, const char **value) {
    const AmdAttr *a = own_attr(attr);
    if (!a || i < 0 || i >= (int)a->kv.size()) return -1;
    *key = a->kv[i].first.c_str(); *value = a->kv[i].second.c_str();
    return 0;
}

void aprilsam_amd_graph_from_arrays(april_graph_t *g, int N, const double *states, int F, const int *fa, const int *fb,
                                    const double *z, const double *W) {
    for (int i = 0; i < N; i++) {
        april_graph_node_t *n = april_graph_node_xyt_create(states + 3 * i, states + 3 * i, states + 3 * i);
        zarray_append(g->nodes, &n);
    }
    matd_t *Wm = matd33(nullptr);
    for (int i = 0; i < F; i++) {
        memcpy(Wm->data, W + 9 * (size_t)i, 72);
        double zz[3] = { z[3 * (size_t)i], z[3 * (size_t)i + 1], z[3 * (size_t)i + 2] };
        april_graph_factor_t *f = fb[i] < 0 ? april_graph_factor_xytpos_create(fa[i], zz, nullptr, Wm)
                                            : april_graph_factor_xyt_create(fa[i], fb[i], zz, nullptr, Wm);
        zarray_append(g->factors, &f);
    }
    free(Wm);
}

// bulk read of the node objects (state / l_point / delta_X, april_graph_xyt.c:302-314 fields): what a checker of a big graph
// needs without a million ctypes round trips; any of the three destinations may be null
void aprilsam_amd_graph_node_arrays(const april_graph_t *g, double *state, double *l_point, double *delta_X) {
    const int N = g && g->nodes ? g->nodes->size : 0;
    april_graph_node_t *const *ns = N ? (april_graph_node_t *const *)g->nodes->data : nullptr;
    for (int i = 0; i < N; i++) {
        const april_graph_node_t *n = ns[i];
        if (state) memcpy(state + 3 * (size_t)i, n->state, 24);
        if (l_point) memcpy(l_point + 3 * (size_t)i, n->l_point, 24);
        if (delta_X) memcpy(delta_X + 3 * (size_t)i, n->delta_X, 24);
    }
}

// ---- synthetic Manhattan lattice, SURVEY.md §8(d) config 4/5 -------------------------------------------
// K x K poses on a unit grid, snake numbering id(r,c) = r*K + (r odd ? K-1-c : c); truth = (c, r, r odd ? pi : 0);
// splitmix64 PRNG (state 0x9E3779B97F4A7C15, first output after state += gamma); u01 = (x >> 11) * 2^-53;
// gauss = sqrt(-2 ln u1) cos(2 pi u2), u1 clamped to >= 1e-300, u1 drawn first.
namespace {
struct SplitMix {
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    unsigned long long next() {
        s += 0x9E3779B97F4A7C15ull;
        unsigned long long z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double u01() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double gauss() {
        double u1 = u01(), u2 = u01();
        if (u1 < 1e-300) u1 = 1e-300;
        return sqrt(-2.0 * log(u1)) * cos(2.0 * 3.141592653589793238462643383279502884196 * u2);
    }
};
}  // namespace

int aprilsam_amd_lattice_arrays(int K, double *states, int *fa, int *fb, double *z, double *W) {
    const double PI_ = 3.141592653589793238462643383279502884196;
    auto id = [&](int r, int c) { return r * K + ((r & 1) ? K - 1 - c : c); };
    const int N = K * K;
    double *truth = (double *)malloc(sizeof(double) * 3 * (size_t)N);
    for (int r = 0; r < K; r++)
        for (int c = 0; c < K; c++) { int i = id(r, c); truth[3 * i] = c; truth[3 * i + 1] = r; truth[3 * i + 2] = (r & 1) ? PI_ : 0.0; }
    SplitMix rng;
    for (int i = 0; i < N; i++) {                 // id ascending; node 0 draws, then is pinned to the origin
        double g0 = rng.gauss(), g1 = rng.gauss(), g2 = rng.gauss();
        states[3 * i] = truth[3 * i] + 0.2 * g0; states[3 * i + 1] = truth[3 * i + 1] + 0.2 * g1; states[3 * i + 2] = truth[3 * i + 2] + 0.05 * g2;
    }
    states[0] = states[1] = states[2] = 0;
    int F = 0;
    const int d[4][2] = { { 0, 1 }, { 1, 0 }, { 1, 1 }, { 1, -1 } };
    for (int r = 0; r < K; r++)
        for (int c = 0; c < K; c++)
            for (int k = 0; k < 4; k++) {
                int r2 = r + d[k][0], c2 = c + d[k][1];
                if (r2 < 0 || r2 >= K || c2 < 0 || c2 >= K) continue;
                int a = id(r, c), b = id(r2, c2);
                if (a > b) { int t = a; a = b; b = t; }
                const double *ta = truth + 3 * a, *tb = truth + 3 * b;
                double ca = cos(ta[2]), sa = sin(ta[2]), dx = tb[0] - ta[0], dy = tb[1] - ta[1];
                double g0 = rng.gauss(), g1 = rng.gauss(), g2 = rng.gauss();
                fa[F] = a; fb[F] = b;
                z[3 * (size_t)F] = (ca * dx + sa * dy) + 0.05 * g0;           // truth_a^-1 o truth_b (doubles_floats_impl.h:619)
                z[3 * (size_t)F + 1] = (-sa * dx + ca * dy) + 0.05 * g1;
                z[3 * (size_t)F + 2] = mod2pi_h((tb[2] - ta[2]) + 0.01 * g2);
                double *w = W + 9 * (size_t)F;
                memset(w, 0, 72); w[0] = 400; w[4] = 400; w[8] = 1e4;
                F++;
            }
    fa[F] = 0; fb[F] = -1;                        // prior on node 0, W = diag(1e4, 1e4, 1e3), z = 0
    z[3 * (size_t)F] = z[3 * (size_t)F + 1] = z[3 * (size_t)F + 2] = 0;
    { double *w = W + 9 * (size_t)F; memset(w, 0, 72); w[0] = 1e4; w[4] = 1e4; w[8] = 1e3; }
    F++;
    free(truth);
    return F;
}

int aprilsam_amd_make_lattice(april_graph_t *g, int K) {
    const size_t N = (size_t)K * K, Fmax = 4 * N + 1;
    double *st = (double *)malloc(24 * N), *z = (double *)malloc(24 * Fmax), *W = (double *)malloc(72 * Fmax);
    int *fa = (int *)malloc(4 * Fmax), *fb = (int *)malloc(4 * Fmax);
    int F = aprilsam_amd_lattice_arrays(K, st, fa, fb, z, W);
    aprilsam_amd_graph_from_arrays(g, (int)N, st, F, fa, fb, z, W);
    free(st); free(z); free(W); free(fa); free(fb);
    return F;
}

}  // extern "C"
