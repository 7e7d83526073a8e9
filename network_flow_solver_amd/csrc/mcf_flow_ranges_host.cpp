// mcf_flow_ranges_host.cpp -- host restatement of the logic of mcf_supply_ranges / mcf_capacity_ranges, test infrastructure only.
//
// The kernels (mcf_passes_dev.h: k_frng_*) call the MCF_HD functions of mcf_core.h (mcf_frng_*, mcf_rng_jumps); this file calls
// the very same functions from plain loops over caller's arrays, so the CPU test-suite can hold them against numpy yardsticks
// on planted trees without a device.  It is NOT a CPU path of the library: nothing in the package loads it.
//
// The order in which the levels are combined differs from any a device run uses, on purpose -- the result may not depend on
// it: with order != 0 every level is built nodes LAST to first, with order == 0 first to last.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcf_core.h"

namespace {

struct Tables {
    int32_t N = 0;
    int K = 1;
    int64_t m = 0;
    const int32_t *pred_arc = nullptr, *depth = nullptr;
    const int8_t* up = nullptr;
    std::vector<int32_t> anc, id[2];
    std::vector<int64_t> val[2];
    int32_t pred(int32_t v) const { return pred_arc[v] < 0 ? -1 : (int32_t)(((int64_t)pred_arc[v] << 1) | (up[v] ? 1 : 0)); }
    int64_t index(int32_t node) const { return node < 0 ? -1 : (int64_t)pred_arc[node]; }
    void push(int32_t x, int32_t y, McfFrngPush* p) const {
        mcf_frng_push(x, y, K, m, [&](int k, int32_t v) { return anc[(size_t)k * N + v]; },
                      [&](int w, int k, int32_t v) { return McfFrngMin{val[w][(size_t)k * N + v], id[w][(size_t)k * N + v]}; },
                      [&](int32_t v) { return depth[v]; }, [&](int32_t v) { return pred(v); }, p);
    }
    void push_both(int32_t t, int32_t hd, McfFrngPush* f, McfFrngPush* b) const {
        mcf_frng_push_both(t, hd, K, m, [&](int k, int32_t v) { return anc[(size_t)k * N + v]; },
                           [&](int w, int k, int32_t v) { return McfFrngMin{val[w][(size_t)k * N + v], id[w][(size_t)k * N + v]}; },
                           [&](int32_t v) { return depth[v]; }, [&](int32_t v) { return pred(v); }, f, b);
    }
};

// node arrays have n + 1 entries, the root is node n.  pred_arc[v]: the caller's index of v's tree arc, m + v for an artificial
// one (mcf_get_tree's layout); up[v]: the arc points v -> parent; tflow[v], tcap[v]: its flow and capacity (>= 2^60 or < 0:
// none; an artificial arc's magnitude and anything).  report[0..4]: basic_real, basic_artificial, 0, max_depth, levels.
void build(Tables* T, int32_t n, int64_t m, const int32_t* parent, const int32_t* pred_arc, const int8_t* up, const int32_t* depth,
           const int64_t* tflow, const int64_t* tcap, int order, int64_t* report) {
    const int32_t N = n + 1;
    int64_t max_depth = 0;
    for (int32_t v = 0; v < n; ++v) if (depth[v] > max_depth) max_depth = depth[v];
    const int K = mcf_rng_levels(max_depth);
    T->N = N; T->K = K; T->m = m; T->pred_arc = pred_arc; T->depth = depth; T->up = up;
    report[3] = max_depth; report[4] = K;
    T->anc.assign((size_t)K * N, 0);
    for (int w = 0; w < 2; ++w) { T->val[w].assign((size_t)K * N, MCF_RNG_INF); T->id[w].assign((size_t)K * N, -1); }
    for (int32_t v = 0; v < N; ++v) {
        T->anc[(size_t)v] = mcf_rng_anc0(v, parent[v], N);
        if (v == n || pred_arc[v] < 0) continue;
        const int64_t cap = (tcap[v] < 0 || tcap[v] >= MCF_INF) ? MCF_INF : tcap[v];
        mcf_frng_residuals(T->pred(v), m, cap, tflow[v], &T->val[0][(size_t)v], &T->val[1][(size_t)v]);
        T->id[0][(size_t)v] = T->id[1][(size_t)v] = v;
        ++report[pred_arc[v] >= m ? 1 : 0];
    }
    for (int k = 1; k < K; ++k) {
        const size_t row = (size_t)k * N, low = row - N;
        for (int32_t i = 0; i < N; ++i) {
            const int32_t v = order ? N - 1 - i : i;
            const int32_t a = T->anc[low + v];
            T->anc[row + v] = T->anc[low + a];
            const McfFrngMin U = mcf_frng_up({T->val[0][low + v], T->id[0][low + v]}, {T->val[0][low + a], T->id[0][low + a]});
            const McfFrngMin D = mcf_frng_down({T->val[1][low + v], T->id[1][low + v]}, {T->val[1][low + a], T->id[1][low + a]});
            T->val[0][row + v] = U.val; T->id[0][row + v] = U.id;
            T->val[1][row + v] = D.val; T->id[1][row + v] = D.id;
        }
    }
}

}  // namespace

extern "C" {

// report[10]: basic_real, basic_artificial, at_capacity, max_depth, levels, inf_count, zero_count, art_rising_count, 0, 0
int mcf_supply_ranges_host(int32_t n, int64_t m, const int32_t* parent, const int32_t* pred_arc, const int8_t* up, const int32_t* depth,
                           const int64_t* tflow, const int64_t* tcap, const int64_t* pi, int order, int64_t count, const int32_t* from, const int32_t* to,
                           int64_t* limit, int64_t* limit_arc, int64_t* rate, int32_t* art_rising, int64_t* report) {
    if (n < 1 || m < 0 || count < 0 || !parent || !pred_arc || !up || !depth || !tflow || !tcap || !pi || !report) return -1;
    if (count > 0 && (!from || !to || !limit || !limit_arc || !rate || !art_rising)) return -1;
    std::memset(report, 0, 10 * sizeof(int64_t));
    Tables T;
    build(&T, n, m, parent, pred_arc, up, depth, tflow, tcap, order, report);
    for (int64_t i = 0; i < count; ++i) {
        if (from[i] < 0 || from[i] >= n || to[i] < 0 || to[i] >= n) return -1;
        McfFrngPush p;
        T.push(from[i], to[i], &p);
        const McfFrngMin r = mcf_frng_end(p);
        limit[i] = r.val; limit_arc[i] = T.index(r.id); rate[i] = pi[to[i]] - pi[from[i]]; art_rising[i] = p.rising;
        report[5] += r.val == MCF_RNG_INF; report[6] += r.val == 0; report[7] += p.rising > 0;
    }
    return 0;
}

// arcs in the caller's order: tail, head, cost, cap (mcf_create's convention), flow, state.  Answers for all m arcs.
int mcf_capacity_ranges_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap, const int64_t* flow,
                             const int8_t* state, const int32_t* parent, const int32_t* pred_arc, const int8_t* up, const int32_t* depth,
                             const int64_t* tflow, const int64_t* tcap, const int64_t* pi, int order,
                             int64_t* down, int64_t* upr, int64_t* down_arc, int64_t* up_arc, int64_t* rate, int64_t* report) {
    if (n < 1 || m < 0 || !parent || !pred_arc || !up || !depth || !tflow || !tcap || !pi || !report) return -1;
    if (m > 0 && (!tail || !head || !cost || !cap || !flow || !state || !down || !upr || !down_arc || !up_arc || !rate)) return -1;
    std::memset(report, 0, 10 * sizeof(int64_t));
    Tables T;
    build(&T, n, m, parent, pred_arc, up, depth, tflow, tcap, order, report);
    for (int64_t f = m; f-- > 0;) {
        const int64_t c = (cap[f] < 0 || cap[f] >= MCF_INF) ? MCF_INF : cap[f];
        int64_t rc = 0;
        McfFrngMin fwd = {MCF_RNG_INF, -1}, back = {MCF_RNG_INF, -1};
        if (mcf_frng_needs_push(state[f], c)) {
            ++report[2];
            rc = cost[f] + pi[tail[f]] - pi[head[f]];
            McfFrngPush pf, pb;
            T.push_both(tail[f], head[f], &pf, &pb);
            fwd = mcf_frng_end(pf);
            back = mcf_frng_end(pb);
            report[7] += (pf.rising > 0) + (pb.rising > 0);
        }
        const McfFrngArc r = mcf_frng_arc(state[f], c, flow[f], rc, f, fwd.val, T.index(fwd.id), back.val, T.index(back.id));
        down[f] = r.down; upr[f] = r.up; down_arc[f] = r.down_arc; up_arc[f] = r.up_arc; rate[f] = r.rate;
        report[5] += (r.down == MCF_RNG_INF) + (r.up == MCF_RNG_INF);
        report[6] += (r.down == 0) + (r.up == 0);
    }
    return 0;
}

}  // extern "C"
