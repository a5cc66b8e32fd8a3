/* Test infrastructure: an independent max-mixture factor (Olson & Agarwal, RSS 2012) written against the public object layout
 * (include/aprilsam_amd.h PART 1 == aprilsam/aprilsam.h:98-146), with its own vtable -- the checker of the library's native max
 * factors.  Its components are whatever factors the caller hands in (the reference's xyt factors when it
 * drives the reference); eval() calls each component's own eval(), scores it as
 *     s_i = eval->chi2 - 2 logw_i - ln det W_i
 * applies the selection loop  best = 0; for i in 1..K-1: if (s_i < s_best) best = i  and returns the winner's evaluation.  It records
 * the winner (mm_last) and the smallest relative score margin any selection had (mm_min_margin).  The type tag is a parameter: with
 * tag 3 (APRILSAM_AMD_FACTOR_MAX_TYPE) on the product library it must still take the host-evaluated path.
 *
 *   gcc -O2 -fPIC -shared -Iinclude tests/support/maxmix_factor.c -o <out>.so -lm
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "aprilsam_amd.h"

typedef struct { int last, last_state; } mm_ext_t;       /* lives right behind the factor object (one calloc) */
static double g_min_margin = INFINITY;
static long long g_evals = 0;

static mm_ext_t *ext_of(const april_graph_factor_t *f) { return (mm_ext_t *)(f + 1); }

static double det3(const double *w) {
    return w[0] * (w[4] * w[8] - w[5] * w[7]) - w[1] * (w[3] * w[8] - w[5] * w[6]) + w[2] * (w[3] * w[7] - w[4] * w[6]);
}

static april_graph_factor_eval_t *mm_eval_at(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e, int at_state) {
    const int n = f->u.max.nfactors;
    int best = 0;
    double sbest = 0, ssecond = INFINITY;
    for (int i = 0; i < n; i++) {         /* (one evaluation object for all: the components are xyt factors of one shape) */
        april_graph_factor_t *c = f->u.max.factors[i];
        e = at_state ? c->state_eval(c, g, e) : c->eval(c, g, e);
        const double s = e->chi2 - 2.0 * f->u.max.logw[i] - log(det3(c->u.common.W->data));
        if (i == 0) sbest = s;
        else if (s < sbest) { ssecond = sbest; best = i; sbest = s; }
        else if (s < ssecond) ssecond = s;
    }
    if (n > 1) {
        const double margin = (ssecond - sbest) / fmax(fabs(sbest), fabs(ssecond));
        if (margin < g_min_margin) g_min_margin = margin;
    }
    g_evals++;
    if (at_state) ext_of(f)->last_state = best; else ext_of(f)->last = best;
    april_graph_factor_t *w = f->u.max.factors[best];
    return at_state ? w->state_eval(w, g, e) : w->eval(w, g, e);
}
static april_graph_factor_eval_t *mm_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return mm_eval_at(f, g, e, 0); }
static april_graph_factor_eval_t *mm_state_eval(april_graph_factor_t *f, april_graph_t *g, april_graph_factor_eval_t *e) { return mm_eval_at(f, g, e, 1); }
static void mm_destroy(april_graph_factor_t *f) {
    for (int i = 0; i < f->u.max.nfactors; i++) f->u.max.factors[i]->destroy(f->u.max.factors[i]);
    free(f->u.max.factors); free(f->u.max.logw); free(f->nodes); free(f);
}
april_graph_factor_t *mm_create(int type, april_graph_factor_t **comps, const double *logw, int n);
static april_graph_factor_t *mm_copy(april_graph_factor_t *f) {
    april_graph_factor_t **cs = (april_graph_factor_t **)calloc((size_t)f->u.max.nfactors, sizeof(*cs));
    for (int i = 0; i < f->u.max.nfactors; i++) cs[i] = f->u.max.factors[i]->copy(f->u.max.factors[i]);
    april_graph_factor_t *c = mm_create(f->type, cs, f->u.max.logw, f->u.max.nfactors);
    free(cs);
    return c;
}

/* takes ownership of comps[0..n) (all on the same node pair); copies logw */
april_graph_factor_t *mm_create(int type, april_graph_factor_t **comps, const double *logw, int n) {
    april_graph_factor_t *f = (april_graph_factor_t *)calloc(1, sizeof(*f) + sizeof(mm_ext_t));
    f->type = type; f->nnodes = 2; f->length = 3;
    f->nodes = (int *)calloc(2, sizeof(int)); f->nodes[0] = comps[0]->nodes[0]; f->nodes[1] = comps[0]->nodes[1];
    f->copy = mm_copy; f->eval = mm_eval; f->state_eval = mm_state_eval; f->destroy = mm_destroy;
    f->u.max.factors = (april_graph_factor_t **)calloc((size_t)n, sizeof(april_graph_factor_t *));
    memcpy(f->u.max.factors, comps, sizeof(april_graph_factor_t *) * (size_t)n);
    f->u.max.logw = (double *)calloc((size_t)n, sizeof(double));
    memcpy(f->u.max.logw, logw, sizeof(double) * (size_t)n);
    f->u.max.nfactors = n;
    ext_of(f)->last = ext_of(f)->last_state = -1;
    return f;
}
int mm_last(const april_graph_factor_t *f) { return ext_of(f)->last; }
int mm_last_state(const april_graph_factor_t *f) { return ext_of(f)->last_state; }
double mm_min_margin(void) { return g_min_margin; }
long long mm_evals(void) { return g_evals; }
void mm_reset_stats(void) { g_min_margin = INFINITY; g_evals = 0; }
