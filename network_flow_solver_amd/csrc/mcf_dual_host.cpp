// mcf_dual_host.cpp -- host restatement of the dual pivots of mcf_update_rhs_dual, test infrastructure only.
//
// The kernels (mcf_passes_dev.h: k_dual_leave, k_dual_enter, k_pivot_dual) call the MCF_HD functions of mcf_core.h
// (mcf_dual_*, mcf_pivot_begin_dual, mcf_pivot_decide_forced, mcf_pivot_finish); this file calls the very same functions from
// plain loops, so the CPU test-suite can hold them against an independent reference without a device:
//   mcf_dual_select_host   the two choices over plain arrays in the caller's order;
//   mcf_dual_run_host      whole dual pivots, one after the other, on a dense host view staged from a McfHostImage.
// It is NOT a CPU path of the library: nothing in the package loads it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_host.h"

namespace {

// chunked reduction in an order no device run uses: chunk accumulators merged last to first when `order` != 0
template <typename Acc, typename Body>
Acc reduce_chunks(int64_t count, int64_t chunk, int order, Body body) {
    std::vector<Acc> part;
    for (int64_t lo = 0; lo < count; lo += chunk) {
        Acc a;
        mcf_acc_init(&a);
        const int64_t hi = lo + chunk < count ? lo + chunk : count;
        for (int64_t i = lo; i < hi; ++i) body(&a, order ? hi - 1 - (i - lo) : i);
        part.push_back(a);
    }
    Acc total;
    mcf_acc_init(&total);
    for (size_t k = 0; k < part.size(); ++k) mcf_acc_merge(&total, part[order ? part.size() - 1 - k : k]);
    return total;
}

struct Run {
    McfHostImage im;
    std::vector<int32_t> order1, path1, path2, pos1, psz1, ppos1, ppos2, reach, chg;
    std::vector<McfNode> rec1, rec2;
    std::vector<McfSeg> seg;
    McfCtx ctx{};
    McfView view{};
};

// the dense view of oracle/emul_engine.cpp's bind(): gathered reduced costs, position-space sizes and coarse index kept
// (scan = true) or not (the climb finds every cycle)
void stage(Run& r, bool scan, int32_t climb_budget) {
    McfHostImage& im = r.im;
    const size_t N = (size_t)im.n_nodes;
    r.order1 = im.order;
    r.pos1 = im.pos;
    r.path1.assign(N, 0); r.path2.assign(N, 0);
    r.ppos1.assign(2 * N, 0); r.ppos2.assign(2 * N, 0);
    r.rec1.assign(N, McfNode{0, 0, 0, 0}); r.rec2.assign(N, McfNode{0, 0, 0, 0});
    r.seg.assign(2 * N + 2, McfSeg{0, 0, 0, 0});
    std::memset(&r.ctx, 0, sizeof r.ctx);
    r.ctx.unbounded_arc = -1;
    r.ctx.status = MCF_RUNNING;
    r.ctx.max_pivots = INT64_MAX;
    r.ctx.climb_budget = climb_budget;
    r.ctx.climb_depth = 0;
    McfView& v = r.view;
    v.n_nodes = im.n_nodes;
    v.m = im.m;
    v.tail = im.tail.data(); v.head = im.head.data(); v.cost = im.cost.data(); v.orig = im.orig.data();
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) v.bucket_off[x] = im.bucket_off[x];
    v.state = im.state.data();
    v.arcw = im.arcw.data();
    v.pi = im.pi.data();
    v.node = im.node.data();
    v.order[0] = im.order.data(); v.order[1] = r.order1.data();
    v.path1 = r.path1.data(); v.path2 = r.path2.data();
    v.ppos1 = r.ppos1.data(); v.ppos2 = r.ppos2.data();
    v.rec1 = r.rec1.data(); v.rec2 = r.rec2.data();
    v.seg = r.seg.data();
    v.ctx = &r.ctx;
    v.vk_bigm = im.big_m; v.vk_half = 1 << 28;
    v.posbuf[0] = im.pos.data(); v.posbuf[1] = r.pos1.data();
    r.chg.assign(N, 0);
    v.chg = r.chg.data();
    if (scan) {
        const size_t np = (N + MCF_REACH_BLOCK - 1) / MCF_REACH_BLOCK * MCF_REACH_BLOCK + 4;
        im.psize.resize(np, 0);
        r.psz1 = im.psize;
        v.psz[0] = im.psize.data(); v.psz[1] = r.psz1.data();
        r.reach.assign(np / MCF_REACH_BLOCK + 8, 0);
        v.reach = r.reach.data();
        for (int32_t b = 0; b < (im.n_nodes + MCF_REACH_BLOCK - 1) / MCF_REACH_BLOCK; ++b) mcf_reach_reindex_block(v, v.psz[0], b);
    }
}

// the apply pass of one pivot on the dense arrays, then the coarse blocks it touched are re-indexed (emul_engine.cpp's)
void apply_all(Run& r) {
    McfCtx& c = r.ctx;
    if (!c.apply) return;
    for (int32_t j = c.lo; j < c.hi; ++j) mcf_apply_one(r.view, c, j);
    for (int32_t j = c.prev_lo; j < c.prev_hi; ++j)
        if (j < c.lo || j >= c.hi) mcf_apply_one(r.view, c, j);
    if (!r.view.reach) return;
    const int32_t* znew = c.cur ? r.view.psz[0] : r.view.psz[1];
    auto range = [&](int32_t lo, int32_t hi) {
        if (hi <= lo) return;
        for (int32_t b = lo >> MCF_REACH_SHIFT; b <= (hi - 1) >> MCF_REACH_SHIFT; ++b) mcf_reach_reindex_block(r.view, znew, b);
    };
    range(c.lo, c.hi);
    range(c.prev_lo, c.prev_hi);
    auto meets = [&](int32_t b, int32_t lo, int32_t hi) { return hi > lo && b >= (lo >> MCF_REACH_SHIFT) && b <= ((hi - 1) >> MCF_REACH_SHIFT); };
    for (int32_t t = 0; t < c.nchg; ++t) {
        const int32_t b = r.view.chg[t] >> MCF_REACH_SHIFT;
        if (meets(b, c.lo, c.hi) || meets(b, c.prev_lo, c.prev_hi)) continue;
        mcf_reach_reindex_block(r.view, znew, b);
    }
}

}  // namespace

extern "C" {

// sizeof of the two structs of include/mcf.h as the C compiler lays them out: 0 = mcf_dual_options, 1 = mcf_dual_report
int64_t mcf_dual_sizeof(int32_t which) { return which == 0 ? (int64_t)sizeof(mcf_dual_options) : (int64_t)sizeof(mcf_dual_report); }

// The two choices over plain arrays.  Arcs in the caller's order: tail, head, cost, cap (>= 2^60 or < 0: none), state.  Node
// arrays have n + 1 entries, the root is node n: pred_arc[v] (caller's index, m + v artificial, -1 root), up[v], tflow[v] /
// tcap[v] (flow and capacity of v's tree arc), pos[v], size[v], pi[v].  order != 0: the reductions run in another order.
// out[8]: q (-1: none), violation, leaving state, exports, entering arc (-1: none), slack, largest |tree flow|, 1 when the
// magnitude limit forbids the pivot (mcf_dual_too_large).
int mcf_dual_select_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                         const int8_t* state, const int32_t* pred_arc, const int8_t* up, const int64_t* tflow, const int64_t* tcap,
                         const int32_t* pos, const int32_t* size, const int64_t* pi, int order, int64_t* out) {
    if (n < 1 || m < 0 || !pred_arc || !up || !tflow || !tcap || !pos || !size || !pi || !out) return -1;
    if (m > 0 && (!tail || !head || !cost || !cap || !state)) return -1;
    auto capof = [](int64_t c) { return (c < 0 || c >= MCF_INF) ? MCF_INF : c; };
    const McfDualLeave L = reduce_chunks<McfDualLeave>(n, 7, order, [&](McfDualLeave* a, int64_t v) {
        if (pred_arc[v] < 0) return;
        mcf_dual_leave_add(a, mcf_dual_violation(capof(tcap[v]), tflow[v]), v, tflow[v]);
    });
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[0] = L.node; out[1] = L.viol; out[4] = -1; out[6] = L.maxabs; out[7] = mcf_dual_too_large(L) ? 1 : 0;
    if (L.node < 0) return 0;
    const int32_t q = (int32_t)L.node;
    const bool exports = mcf_dual_exports(up[q] != 0, tflow[q]);
    out[2] = mcf_dual_leave_state(tflow[q]);
    out[3] = exports ? 1 : 0;
    const McfDualEnter E = reduce_chunks<McfDualEnter>(m, 5, order, [&](McfDualEnter* a, int64_t e) {
        const bool tin = mcf_dual_in_subtree(pos[tail[e]], pos[q], size[q]), hin = mcf_dual_in_subtree(pos[head[e]], pos[q], size[q]);
        if (!mcf_dual_candidate(state[e], capof(cap[e]), tin, hin, exports)) return;
        mcf_dual_enter_add(a, (int64_t)state[e] * (cost[e] + pi[tail[e]] - pi[head[e]]), mcf_pack_arc((int32_t)e, e));
    });
    out[4] = E.arc < 0 ? -1 : (E.arc >> 32);
    out[5] = E.arc < 0 ? 0 : E.slack;
    return 0;
}

// Whole dual pivots on the host.  The instance (caller's arc order) with its OLD supplies / capacities and a basis that fits
// them (as for mcf_set_basis) is installed by mcf_apply_basis; then new_supply[n] / new_cap[m] take their place the way the
// device passes of mcf_update_rhs apply an edit (a non-basic arc at capacity follows its capacity, or goes back to its lower
// bound when that is 0 or none; tree flows are subtree sums of the balances), and dual pivots run one after the other:
// mcf_pivot_begin_dual, climb (and scan, climb_budget >= 0), mcf_pivot_decide_forced, mcf_pivot_finish, the sequential apply.
// Outputs (n + 1 node entries, root = n): start_pred[n+1] / start_up[n+1] / start_state[m]: the basis the run starts from;
// log[4 * log_cap]; parent, pred_arc (caller's index, m + v, -1), up, size, depth, pos; state[m], flow[m], art_flow[n],
// pi[n+1]; report[4] = ended (0 cleared, 1 no entering arc, 2 budget, 3 not attempted, 4 magnitude), reason (3 / 4 as in
// mcf_dual_report), dual pivots, violations at the start.  Returns 0, 1 when the basis was refused (err), -1 on bad arguments,
// -2 on an internal error of the pivot.
int mcf_dual_run_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                      const int64_t* supply, const int8_t* in_tree, const int8_t* at_upper, const int64_t* new_supply, const int64_t* new_cap,
                      int64_t max_pivots, int32_t climb_budget, int32_t* start_pred, int8_t* start_up, int8_t* start_state,
                      int64_t* log, int64_t log_cap, int32_t* parent, int32_t* pred_arc, int8_t* up, int32_t* size, int32_t* depth, int32_t* pos,
                      int8_t* state, int64_t* flow, int64_t* art_flow, int64_t* pi, int64_t* report, char* err, int32_t err_len) {
    auto say = [&](const std::string& s) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", s.c_str()); };
    if (!new_supply || !report || (m > 0 && !new_cap) || log_cap < 0 || (log_cap > 0 && !log)) return -1;
    Run r;
    McfHostImage& im = r.im;
    int code = 0;
    const std::string bad = mcf_build_image(n, m, tail, head, cost, cap, supply, im, &code);
    if (!bad.empty()) { say(bad); return -1; }
    const std::string msg = mcf_apply_basis(im, in_tree, at_upper);
    if (!msg.empty()) { say(msg); return 1; }
    const int32_t N = im.n_nodes;
    for (int32_t v = 0; v <= n; ++v) {
        const McfNode nd = im.node[(size_t)v];
        const int64_t a = nd.pred < 0 ? -1 : nd.pred >> 1;
        if (start_pred) start_pred[v] = a < 0 ? -1 : (a < m ? im.orig[(size_t)a] : (int32_t)a);
        if (start_up) start_up[v] = nd.pred < 0 ? 0 : (int8_t)(nd.pred & 1);
    }
    if (start_state) for (int64_t e = 0; e < m; ++e) start_state[im.orig[(size_t)e]] = im.state[(size_t)e];
    // ---- the edit
    for (int32_t v = 0; v < n; ++v) im.supply[(size_t)v] = new_supply[v];
    for (int64_t e = 0; e < m; ++e) {
        const int64_t c = new_cap[im.orig[(size_t)e]];
        const int64_t nc = (c < 0 || c >= MCF_INF) ? MCF_INF : c;
        McfArcW& w = im.arcw[(size_t)e];
        if (w.cap == nc) continue;
        w.cap = nc;
        if (im.state[(size_t)e] == -1) {
            if (nc >= MCF_INF || nc == 0) { im.state[(size_t)e] = 1; w.flow = 0; } else w.flow = nc;
        }
    }
    std::vector<__int128> bal((size_t)N, 0);
    for (int32_t v = 0; v < n; ++v) bal[(size_t)v] = im.supply[(size_t)v];
    for (int64_t e = 0; e < m; ++e) {
        if (im.state[(size_t)e] == 0) continue;
        bal[(size_t)im.tail[(size_t)e]] -= im.arcw[(size_t)e].flow;
        bal[(size_t)im.head[(size_t)e]] += im.arcw[(size_t)e].flow;
    }
    int64_t violations = 0, flips = 0, huge = 0;
    for (int32_t k = N - 1; k >= 1; --k) {
        const int32_t v = im.order[(size_t)k];
        const McfNode nd = im.node[(size_t)v];
        const __int128 x = bal[(size_t)v];
        const int64_t a = nd.pred >> 1;
        const bool isup = (nd.pred & 1) != 0;
        if (a < m) {
            const __int128 f = isup ? x : -x;
            if (f <= -(__int128)MCF_INF || f >= (__int128)MCF_INF) { ++huge; ++violations; }
            else {
                im.arcw[(size_t)a].flow = (int64_t)f;
                if (mcf_dual_violation(im.arcw[(size_t)a].cap, (int64_t)f) > 0) ++violations;
            }
        } else {
            const __int128 ax = x < 0 ? -x : x;
            if (ax >= (__int128)MCF_INF) { ++huge; ++violations; }
            else {
                im.arcw[(size_t)a].flow = (int64_t)ax;
                if ((x >= 0) != isup && ax != 0) ++flips;
            }
        }
        bal[(size_t)nd.parent] += x;
    }
    report[0] = 3; report[1] = 0; report[2] = 0; report[3] = violations;
    int64_t bad_slack = 0;
    for (int64_t e = 0; e < m; ++e) {
        const int64_t rc = (int64_t)im.cost[(size_t)e] + im.pi[(size_t)im.tail[(size_t)e]] - im.pi[(size_t)im.head[(size_t)e]];
        if ((int64_t)im.state[(size_t)e] * rc < 0) ++bad_slack;
    }
    if (violations == 0) report[1] = 1;
    else if (flips > 0) report[1] = 4;
    else if (huge > 0) report[1] = 5;
    else if (bad_slack > 0) report[1] = 3;
    int rc_out = 0;
    if (report[1] == 0) {
        stage(r, climb_budget >= 0, climb_budget);
        const McfView& v = r.view;
        McfCtx& c = r.ctx;
        int64_t pivots = 0, ended = 2;
        while (true) {
            const int32_t cur = c.cur ^ (c.pending_flip ? 1 : 0);
            const int32_t* ps = cur ? v.posbuf[1] : v.posbuf[0];
            McfDualLeave L;
            mcf_acc_init(&L);
            for (int32_t u = 0; u < n; ++u) {
                const McfArcW w = v.arcw[v.node[u].pred >> 1];
                mcf_dual_leave_add(&L, mcf_dual_violation(w.cap, w.flow), u, w.flow);
            }
            if (L.node < 0) { ended = 0; break; }
            if (mcf_dual_too_large(L)) { ended = 4; break; }
            if (pivots >= max_pivots) { ended = 2; break; }
            const int32_t q = (int32_t)L.node;
            const McfNode rq = v.node[q];
            const int64_t qflow = v.arcw[rq.pred >> 1].flow;
            const bool exports = mcf_dual_exports((rq.pred & 1) != 0, qflow);
            McfDualEnter E;
            mcf_acc_init(&E);
            for (int64_t e = 0; e < m; ++e) {
                const int32_t st = v.state[e];
                if (st == 0) continue;
                const bool tin = mcf_dual_in_subtree(ps[v.tail[e]], ps[q], rq.size), hin = mcf_dual_in_subtree(ps[v.head[e]], ps[q], rq.size);
                if (!mcf_dual_candidate(st, v.arcw[e].cap, tin, hin, exports)) continue;
                mcf_dual_enter_add(&E, (int64_t)st * ((int64_t)v.cost[e] + v.pi[v.tail[e]] - v.pi[v.head[e]]), mcf_pack_arc(v.orig[e], e));
            }
            if (E.arc < 0) { ended = 1; break; }
            McfCycle cy;
            mcf_pivot_begin_dual(v, E.arc, &cy);
            int32_t slot = 0;
            const int32_t pq = mcf_node_pos(v, &c, q, &slot);
            const bool fin = mcf_dual_in_subtree(mcf_node_pos(v, &c, c.pv_first, &slot), pq, rq.size);
            const McfPaths gp = mcf_view_paths(v);
            if (!mcf_pivot_climb(v, gp, &cy, mcf_climb_budget(v, cy))) { rc_out = -2; break; }
            if (cy.u != cy.w) {
                McfScanAcc acc;
                mcf_scan_init(&acc);
                mcf_pivot_scan(v, gp, 0, &cy, &acc, nullptr, 0, 0, 1);
                if (c.status != MCF_RUNNING || cy.u != cy.w) { rc_out = -2; break; }
            }
            if (pivots < log_cap) {
                const int64_t la = rq.pred >> 1;
                log[4 * pivots] = la < m ? (int64_t)v.orig[la] : la;
                log[4 * pivots + 1] = E.arc >> 32;
                log[4 * pivots + 2] = L.viol;
                log[4 * pivots + 3] = E.slack;
            }
            mcf_pivot_decide_forced(v, gp, cy, q, rq.depth, fin, L.viol, mcf_dual_leave_state(qflow));
            if (c.status != MCF_RUNNING || c.stage != 2) { rc_out = -2; break; }
            mcf_pivot_finish(v, gp, 0, 1);
            apply_all(r);
            ++pivots;
        }
        for (int64_t e = 0; e < m; ++e)   // the end of the phase: closed arcs take the state their reduced cost asks for
            im.state[(size_t)e] = (int8_t)mcf_dual_closed_state(im.state[(size_t)e], im.arcw[(size_t)e].cap,
                                                               (int64_t)im.cost[(size_t)e] + im.pi[(size_t)im.tail[(size_t)e]] - im.pi[(size_t)im.head[(size_t)e]]);
        report[0] = ended; report[2] = pivots;
        if (c.pending_flip) { McfCycle cy; mcf_pivot_begin_dual(v, -1, &cy); }   // the arrays below are read from the current copy
        const int32_t* ps = c.cur ? v.posbuf[1] : v.posbuf[0];
        if (pos) for (int32_t u = 0; u <= n; ++u) pos[u] = ps[u];
    } else if (pos) {
        for (int32_t u = 0; u <= n; ++u) pos[u] = im.pos[(size_t)u];
    }
    for (int32_t u = 0; u <= n; ++u) {
        const McfNode nd = im.node[(size_t)u];
        const int64_t a = nd.pred < 0 ? -1 : nd.pred >> 1;
        if (parent) parent[u] = nd.parent;
        if (pred_arc) pred_arc[u] = a < 0 ? -1 : (a < m ? im.orig[(size_t)a] : (int32_t)a);
        if (up) up[u] = nd.pred < 0 ? 0 : (int8_t)(nd.pred & 1);
        if (size) size[u] = nd.size;
        if (depth) depth[u] = nd.depth;
        if (pi) pi[u] = im.pi[(size_t)u];
    }
    for (int64_t e = 0; e < m; ++e) {
        if (state) state[im.orig[(size_t)e]] = im.state[(size_t)e];
        if (flow) flow[im.orig[(size_t)e]] = im.arcw[(size_t)e].flow;
    }
    if (art_flow) for (int32_t u = 0; u < n; ++u) art_flow[u] = im.arcw[(size_t)(m + u)].flow;
    return rc_out;
}

}  // extern "C"
