// mcf_repair_host.cpp -- mcf_repair_basis and mcf_apply_basis (mcf_host.h) behind plain C functions, test infrastructure only.
//
// mcf_update_rhs repairs a basis on the host when the device census finds tree flows outside their bounds (path 1).  That
// repair is host code and needs no device: this file lets the CPU test-suite run it on arbitrary forests and hold the
// result against numpy.  Nothing in the package loads it.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mcf_host.h"

extern "C" {

// Instance in the caller's arc order (as for mcf_create), basis as for mcf_set_basis, hang[n] as mcf_repair_basis takes it
// (may be null).  Outputs (any may be null): parent[n+1], pred_arc[n+1] (caller's arc index, m + v for the artificial arc
// of node v, -1 for the root), up[n+1] (1: the node is the tail of its tree arc), order[n+1] (preorder), state[m] and
// flow[m] in the caller's arc order, art_flow[n], report[4] = violations, wrong_way, arcs_cut, rounds.
// Returns 0, 1 when the repair refused the basis (text in err), -1 on bad arguments.
int mcf_repair_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                    const int64_t* supply, const int8_t* in_tree, const int8_t* at_upper, const int8_t* hang,
                    int32_t* parent, int32_t* pred_arc, int8_t* up, int32_t* order, int8_t* state, int64_t* flow,
                    int64_t* art_flow, int64_t* report, char* err, int32_t err_len) {
    auto say = [&](const std::string& s) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", s.c_str()); };
    McfHostImage im;
    int code = 0;
    const std::string bad = mcf_build_image(n, m, tail, head, cost, cap, supply, im, &code);
    if (!bad.empty()) { say(bad); return -1; }
    McfRepairReport rr;
    const std::string msg = mcf_repair_basis(im, in_tree, at_upper, hang, &rr);
    if (!msg.empty()) { say(msg); return 1; }
    for (int32_t v = 0; v <= n; ++v) {
        const McfNode nd = im.node[(size_t)v];
        const int64_t a = nd.pred < 0 ? -1 : nd.pred >> 1;
        if (parent) parent[v] = nd.parent;
        if (pred_arc) pred_arc[v] = a < 0 ? -1 : (a < m ? im.orig[(size_t)a] : (int32_t)a);
        if (up) up[v] = nd.pred < 0 ? 0 : (int8_t)(nd.pred & 1);
        if (order) order[v] = im.order[(size_t)v];
    }
    for (int64_t e = 0; e < m; ++e) {
        if (state) state[im.orig[(size_t)e]] = im.state[(size_t)e];
        if (flow) flow[im.orig[(size_t)e]] = im.arcw[(size_t)e].flow;
    }
    if (art_flow) for (int32_t v = 0; v < n; ++v) art_flow[v] = im.arcw[(size_t)(m + v)].flow;
    if (report) { report[0] = rr.violations; report[1] = rr.wrong_way; report[2] = rr.arcs_cut; report[3] = rr.rounds; }
    return 0;
}

// mcf_apply_basis (what mcf_set_basis runs on the host) on the caller's instance and basis.  Outputs (any may be null):
// state[m] and flow[m] in the caller's arc order, art_flow[n].  Returns 0 when the basis was installed; 1 when it was refused
// (text in err): the outputs then show the cold start mcf_set_basis falls back to; -1 on bad arguments.
int mcf_apply_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                   const int64_t* supply, const int8_t* in_tree, const int8_t* at_upper, int8_t* state, int64_t* flow,
                   int64_t* art_flow, char* err, int32_t err_len) {
    auto say = [&](const std::string& s) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", s.c_str()); };
    McfHostImage im;
    int code = 0;
    const std::string bad = mcf_build_image(n, m, tail, head, cost, cap, supply, im, &code);
    if (!bad.empty()) { say(bad); return -1; }
    const std::string msg = mcf_apply_basis(im, in_tree, at_upper);
    if (!msg.empty()) { mcf_init_cold_basis(im); say(msg); }
    for (int64_t e = 0; e < m; ++e) {
        if (state) state[im.orig[(size_t)e]] = im.state[(size_t)e];
        if (flow) flow[im.orig[(size_t)e]] = im.arcw[(size_t)e].flow;
    }
    if (art_flow) for (int32_t v = 0; v < n; ++v) art_flow[v] = im.arcw[(size_t)(m + v)].flow;
    return msg.empty() ? 0 : 1;
}

}  // extern "C"
