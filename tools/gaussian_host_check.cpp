// gaussian_host_check.cpp -- stand-alone check of the dense Gaussian factor's host objects and of aprilsam_amd_graph_remove_nodes
//  under the sanitizers, leak detection on:
//     g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread
//         tools/gaussian_host_check.cpp aprilsam_amd/csrc/{capi,host_objects,ordering,symbolic,refmodel,graph_io,errors}.cpp
//         tests/support/solver_nodevice.cpp -o build/gaussian_host_check && build/gaussian_host_check
// Creates, evaluates (every rank against every node count: the evaluation's Jacobians are freed by april_graph_factor_eval_destroy, which
// frees min(length, k) of them), edits, copies and destroys factors, refuses bad arguments, and edits a graph that holds every factor
// family; exits 0 and prints "ok" when every answer is the documented one (the sanitizers end the run on their own findings).  No device,
// nothing loaded into an interpreter.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/aprilsam_amd.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "gaussian_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// Lambda = J'J for `rank` rows J of a fixed pattern (n = 3k columns), eta = Lambda v
static void make(int k, int rank, std::vector<double> &xbar, std::vector<double> &eta, std::vector<double> &L) {
    const int n = 3 * k;
    std::vector<double> J((size_t)rank * n);
    for (int r = 0; r < rank; r++)
        for (int c = 0; c < n; c++) J[(size_t)r * n + c] = (r == c ? 3.0 : 0.0) + std::sin(1.0 + 0.7 * r + 1.3 * c);
    xbar.assign(n, 0.0); eta.assign(n, 0.0); L.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++)
        for (int j = i; j < n; j++) {
            double a = 0;
            for (int r = 0; r < rank; r++) a += J[(size_t)r * n + i] * J[(size_t)r * n + j];
            L[(size_t)i * n + j] = L[(size_t)j * n + i] = a;
        }
    for (int i = 0; i < n; i++) {
        xbar[i] = 0.1 * i;
        for (int j = 0; j < n; j++) eta[i] += L[(size_t)i * n + j] * (0.05 * (j % 4) - 0.05);
    }
}

int main() {
    april_graph_t *g = april_graph_create();
    for (int i = 0; i < 12; i++) {
        const double p[3] = { 0.3 * i, -0.2 * i, 0.25 * i };
        aprilsam_amd_graph_add_node(g, april_graph_node_xyt_create(p, p, p));
    }
    std::vector<double> xbar, eta, L;
    int nodes[11] = { 7, 0, 11, 3, 9, 1, 5, 10, 2, 8, 4 };
    // every node count against ranks below, at and above it: eval, state_eval, reuse of an evaluation, copy, destroy
    for (int k : { 1, 2, 3, 11 })
        for (int rank : { 0, 1, k - 1, k, k + 1, 3 * k }) {
            if (rank < 0 || rank > 3 * k) continue;
            make(k, rank, xbar, eta, L);
            april_graph_factor_t *f = aprilsam_amd_factor_gaussian_create(k, nodes, xbar.data(), eta.data(), L.data());
            CHECK(f != nullptr && f->type == APRILSAM_AMD_FACTOR_GAUSSIAN_TYPE && f->nnodes == k && f->length == rank);
            int kk = -1;
            CHECK(aprilsam_amd_factor_get_gaussian(f, &kk) == 0 && kk == k);
            april_graph_factor_eval_t *e = f->eval(f, g, nullptr);
            CHECK(e != nullptr && e->length == rank && e->jacobians[k] == nullptr && e->chi2 >= 0);
            for (int i = 0; i < k; i++) CHECK((int)e->jacobians[i]->nrows == rank && e->jacobians[i]->ncols == 3);
            CHECK(f->state_eval(f, g, e) == e);                                    // an evaluation handed back is used again
            // J'J = Lambda to rounding
            const int n = 3 * k;
            double worst = 0, big = 1;
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) {
                    double a = 0;
                    for (int r = 0; r < rank; r++) a += e->jacobians[i / 3]->data[r * 3 + i % 3] * e->jacobians[j / 3]->data[r * 3 + j % 3];
                    worst = std::fmax(worst, std::fabs(a - L[(size_t)i * n + j])); big = std::fmax(big, std::fabs(L[(size_t)i * n + j]));
                }
            CHECK(worst <= 1e-11 * big);
            april_graph_factor_eval_destroy(e);
            april_graph_factor_t *c = f->copy(f);
            CHECK(c != nullptr && c != f && c->u.common.impl != f->u.common.impl && c->u.common.z != f->u.common.z && c->length == rank);
            f->u.common.z[n] += 0.25;                                              // eta edited in place: factorised again at the next evaluation
            e = f->eval(f, g, nullptr);
            CHECK(e != nullptr && e->length == rank);
            april_graph_factor_eval_destroy(e);
            if (n > 1) {
                f->u.common.W->data[1] += 1.0;                                     // no longer symmetric: the evaluation is refused
                CHECK(f->eval(f, g, nullptr) == nullptr);
                f->u.common.W->data[1] -= 1.0;
                e = f->eval(f, g, nullptr);
                CHECK(e != nullptr);
                april_graph_factor_eval_destroy(e);
            }
            f->destroy(f);
            e = c->eval(c, g, nullptr);                                            // the copy outlives the original
            CHECK(e != nullptr && e->length == rank);
            april_graph_factor_eval_destroy(e);
            c->destroy(c);
        }
    // refusals: nothing is owned afterwards
    make(2, 6, xbar, eta, L);
    CHECK(aprilsam_amd_factor_gaussian_create(0, nodes, xbar.data(), eta.data(), L.data()) == nullptr);
    CHECK(aprilsam_amd_factor_gaussian_create(12, nodes, xbar.data(), eta.data(), L.data()) == nullptr);
    CHECK(aprilsam_amd_factor_gaussian_create(2, nullptr, xbar.data(), eta.data(), L.data()) == nullptr);
    int twice[2] = { 4, 4 };
    CHECK(aprilsam_amd_factor_gaussian_create(2, twice, xbar.data(), eta.data(), L.data()) == nullptr);
    L[1] += 1.0;
    CHECK(aprilsam_amd_factor_gaussian_create(2, nodes, xbar.data(), eta.data(), L.data()) == nullptr);       // asymmetric
    L[1] -= 1.0; L[0] = -1.0;
    CHECK(aprilsam_amd_factor_gaussian_create(2, nodes, xbar.data(), eta.data(), L.data()) == nullptr);       // a negative diagonal
    CHECK(aprilsam_amd_factor_get_gaussian(nullptr, nullptr) == 0);
    // the graph edit, on a graph with every family
    const double z[3] = { 0.3, -0.2, 0.25 };
    matd_t *W = (matd_t *)calloc(1, sizeof(matd_t) + 9 * sizeof(double));
    W->nrows = W->ncols = 3; W->data[0] = W->data[4] = W->data[8] = 10.0;
    double z0[3] = { 0, 0, 0 };
    aprilsam_amd_graph_add_factor(g, april_graph_factor_xytpos_create(0, z0, nullptr, W));
    for (int i = 0; i < 11; i++) aprilsam_amd_graph_add_factor(g, april_graph_factor_xyt_create(i, i + 1, z, nullptr, W));
    april_graph_factor_t *comps[2] = { april_graph_factor_xyt_create(2, 9, z, nullptr, W), april_graph_factor_xyt_create(2, 9, z0, nullptr, W) };
    const double logw[2] = { 0.0, -1.0 };
    april_graph_factor_t *mx = aprilsam_amd_factor_max_create(comps, logw, 2);
    CHECK(mx != nullptr);
    aprilsam_amd_graph_add_factor(g, mx);
    const double zp[1] = { 2.0 }, Wp[1] = { 4.0 };
    aprilsam_amd_graph_add_factor(g, aprilsam_amd_factor_polar_create(APRILSAM_AMD_POLAR_RANGE, 10, 6, zp, Wp));
    make(3, 6, xbar, eta, L);
    int tri[3] = { 8, 1, 5 }, touch[3] = { 6, 4, 0 };
    aprilsam_amd_graph_add_factor(g, aprilsam_amd_factor_gaussian_create(3, tri, xbar.data(), eta.data(), L.data()));
    aprilsam_amd_graph_add_factor(g, aprilsam_amd_factor_gaussian_create(3, touch, xbar.data(), eta.data(), L.data()));
    free(W);
    const int F0 = g->factors->size;
    std::vector<int> idx(12, -7);
    int bad[2] = { 3, 12 }, dup[3] = { 3, 4, 3 }, rm[2] = { 4, 3 };
    CHECK(aprilsam_amd_graph_remove_nodes(g, 2, bad, idx.data()) == -13 && aprilsam_amd_graph_remove_nodes(g, 3, dup, idx.data()) == -13);
    CHECK(g->nodes->size == 12 && g->factors->size == F0 && idx[0] == -7);
    CHECK(aprilsam_amd_graph_remove_nodes(g, 2, rm, idx.data()) == 0);
    CHECK(g->nodes->size == 10 && idx[2] == 2 && idx[3] == -1 && idx[4] == -1 && idx[5] == 3 && idx[11] == 9);
    CHECK(g->factors->size == F0 - 3 - 1);                                         // the odometry (2,3), (3,4), (4,5) and the Gaussian factor on (6, 4, 0)
    april_graph_factor_t **fs = (april_graph_factor_t **)g->factors->data;
    april_graph_factor_t *m2 = fs[g->factors->size - 3];
    CHECK(m2->type == APRILSAM_AMD_FACTOR_MAX_TYPE && m2->nodes[0] == 2 && m2->nodes[1] == 7);
    CHECK(m2->u.max.factors[0]->nodes[1] == 7 && m2->u.max.factors[1]->nodes[0] == 2);
    april_graph_factor_t *t2 = fs[g->factors->size - 1];
    int k3 = 0;
    CHECK(aprilsam_amd_factor_get_gaussian(t2, &k3) == 0 && k3 == 3 && t2->nodes[0] == 6 && t2->nodes[1] == 1 && t2->nodes[2] == 3);
    april_graph_factor_eval_t *e = t2->eval(t2, g, nullptr);
    CHECK(e != nullptr);
    april_graph_factor_eval_destroy(e);
    CHECK(aprilsam_amd_graph_remove_nodes(g, 0, nullptr, idx.data()) == 0 && idx[9] == 9);
    april_graph_destroy(g);
    printf("ok\n");
    return 0;
}
