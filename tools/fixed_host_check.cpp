// fixed_host_check.cpp -- stand-alone check of the fixed-node host objects under the sanitizers, leak detection on:
//     g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread
//         tools/fixed_host_check.cpp aprilsam_amd/csrc/{capi,host_objects,ordering,symbolic,refmodel,graph_io,errors}.cpp
//         tests/support/solver_nodevice.cpp -o build/fixed_host_check && build/fixed_host_check
// Creates, fixes, copies, clears and destroys nodes and a graph; exits 0 and prints "ok" when every answer is the documented one (the
// sanitizers end the run on their own findings).  No device, nothing loaded into an interpreter.
#include <cstdio>
#include <cstdlib>

#include "../include/aprilsam_amd.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "fixed_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
    const double s[3] = { 1.0, 2.0, 0.5 };
    // one node: set, get, copy (deep), clear, destroy in every order
    april_graph_node_t *n = april_graph_node_xyt_create(s, s, s);
    CHECK(n->impl == nullptr && aprilsam_amd_node_get_fixed(n) == 0);
    CHECK(aprilsam_amd_node_set_fixed(n, 1) == 0 && n->impl != nullptr && aprilsam_amd_node_get_fixed(n) == 1);
    CHECK(aprilsam_amd_node_set_fixed(n, 1) == 0 && aprilsam_amd_node_get_fixed(n) == 1);          // (twice: one block)
    april_graph_node_t *c = n->copy(n);
    CHECK(c->impl != nullptr && c->impl != n->impl && aprilsam_amd_node_get_fixed(c) == 1);
    CHECK(aprilsam_amd_node_set_fixed(n, 0) == 0 && n->impl == nullptr && aprilsam_amd_node_get_fixed(n) == 0);
    CHECK(aprilsam_amd_node_get_fixed(c) == 1);                                                   // the copy keeps its own
    april_graph_node_t *c2 = n->copy(n);
    CHECK(c2->impl == nullptr);
    n->destroy(n);             // after set and clear
    c->destroy(c);             // after set: destroy frees the block
    c2->destroy(c2);
    // refusals
    CHECK(aprilsam_amd_node_set_fixed(nullptr, 1) == -13 && aprilsam_amd_node_get_fixed(nullptr) == 0);
    n = april_graph_node_xyt_create(s, s, s);
    CHECK(aprilsam_amd_node_set_fixed(n, 2) == -13 && aprilsam_amd_node_set_fixed(n, -1) == -13 && n->impl == nullptr);
    unsigned long long foreign[2] = { 0x1234, 0 };
    n->impl = foreign;
    CHECK(aprilsam_amd_node_set_fixed(n, 1) == -12 && aprilsam_amd_node_set_fixed(n, 0) == -12 && n->impl == foreign && aprilsam_amd_node_get_fixed(n) == 0);
    n->impl = nullptr;
    n->type = 7;
    CHECK(aprilsam_amd_node_set_fixed(n, 1) == -12 && n->impl == nullptr);
    n->type = APRIL_GRAPH_NODE_XYT_TYPE;
    n->destroy(n);
    // a graph: fixed nodes die with it
    april_graph_t *g = april_graph_create();
    for (int i = 0; i < 5; i++) {
        const double p[3] = { (double)i, 0.0, 0.0 };
        april_graph_node_t *q = april_graph_node_xyt_create(p, p, p);
        if (i % 2 == 0) CHECK(aprilsam_amd_node_set_fixed(q, 1) == 0);
        aprilsam_amd_graph_add_node(g, q);
    }
    april_graph_node_t **ns = (april_graph_node_t **)g->nodes->data;
    CHECK(aprilsam_amd_node_get_fixed(ns[0]) == 1 && aprilsam_amd_node_get_fixed(ns[1]) == 0 && aprilsam_amd_node_get_fixed(ns[4]) == 1);
    CHECK(aprilsam_amd_node_set_fixed(ns[2], 0) == 0);
    april_graph_destroy(g);
    printf("ok\n");
    return 0;
}
