/* Test infrastructure: an independent robust-loss factor written against the public object layout (include/aprilsam_amd.h PART 1 ==
 * aprilsam/aprilsam.h:98-146), with its own vtable -- the checker of the library's robust xyt / xytpos factors.
 * It wraps whatever factor the caller hands in (the reference's own xyt factor when it drives the reference); eval() / state_eval()
 * call the inner factor's, take s = eval->chi2 and return the same r and J with W scaled by w(s) and chi2 = rho(s):
 *     1 Huber   w = s <= c^2 ? 1 : c / sqrt(s)
 *     2 Cauchy  w = 1 / (1 + s / c^2)
 *     3 DCS     w = s <= c^2 ? 1 : 4 c^4 / (s + c^2)^2
 * The formulas are written out here on their own, not taken from the library.
 *
 *   gcc -O2 -fPIC -shared -Iinclude tests/support/robust_factor.c -o <out>.so -lm
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "aprilsam_amd.h"

typedef struct { april_graph_factor_t *inner; int kind; double c, last_w; } rb_ext_t;    /* right behind the factor object (one calloc) */
static long long g_evals = 0;

static rb_ext_t *ext_of(const april_graph_factor_t *f) { return (rb_ext_t *)(f + 1); }

static double rb_w(int kind, double c, double s) {
    const double p = c * c;
    if (kind == 1) return s <= p ? 1.0 : c / sqrt(s);
    if (kind == 2) return 1.0 / (1.0 + s / p);
    if (kind == 3) return s <= p ? 1.0 : 4.0 * p * p / ((s + p) * (s + p));
    return 1.0;
}
static double rb_rho(int kind, double c, double s) {
    const double p = c * c;
    if (kind == 1) return s <= p ? s : 2.0 * c * sqrt(s) - p;
    if (kind == 2) return p * log1p(s / p);
    if (kind == 3) return s <= p ? s : p * (3.0 * s - p) / (s + p);
    return s;
}

static april_graph_factor_eval_t *rb_eval_at(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e, int at_state) {
    rb_ext_t *x = ext_of(f);
    april_graph_factor_t *in = x->inner;
    e = at_state ? in->state_eval(in, g, e) : in->eval(in, g, e);
    const double s = e->chi2, w = rb_w(x->kind, x->c, s);
    for (int i = 0; i < 9; i++) e->W->data[i] *= w;
    e->chi2 = rb_rho(x->kind, x->c, s);
    if (!at_state) x->last_w = w;
    g_evals++;
    return e;
}
static april_graph_factor_eval_t *rb_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return rb_eval_at(f, g, e, 0); }
static april_graph_factor_eval_t *rb_state_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return rb_eval_at(f, g, e, 1); }
static void rb_destroy(april_graph_factor_t *f) {
    april_graph_factor_t *in = ext_of(f)->inner;
    in->destroy(in);
    free(f->nodes); free(f);
}
april_graph_factor_t *rb_create(int type, april_graph_factor_t *inner, int kind, double c);
static april_graph_factor_t *rb_copy(april_graph_factor_t *f) {
    return rb_create(f->type, ext_of(f)->inner->copy(ext_of(f)->inner), ext_of(f)->kind, ext_of(f)->c);
}

/* takes ownership of inner (a unary or binary factor) */
april_graph_factor_t *rb_create(int type, april_graph_factor_t *inner, int kind, double c) {
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(*f) + sizeof(rb_ext_t));
    f->type = type; f->nnodes = inner->nnodes; f->length = inner->length;
    f->nodes = (int *)calloc((size_t)inner->nnodes, sizeof(int));
    memcpy(f->nodes, inner->nodes, sizeof(int) * (size_t)inner->nnodes);
    f->copy = rb_copy; f->eval = rb_eval; f->state_eval = rb_state_eval; f->destroy = rb_destroy;
    ext_of(f)->inner = inner; ext_of(f)->kind = kind; ext_of(f)->c = c; ext_of(f)->last_w = -1.0;
    return f;
}
double rb_last_w(const april_graph_factor_t *f) { return ext_of(f)->last_w; }
long long rb_evals(void) { return g_evals; }
