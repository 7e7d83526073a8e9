// mcf_apply_paths_host.cpp -- host twin run of the two back halves of a pivot, test infrastructure only.
//
// The fused LDS loop (mcf_engine.hip: solve_small_body) runs the finish pass and the apply pass of one pivot between the same two
// barriers: mcf_pivot_finish_t<true> writes no segment table and leaves the depth word of the re-hung stem alone, and the apply
// pass takes its sources from the recorded stem (mcf_apply_source_paths, mcf_apply_one_paths).  This file runs whole host pivots
// twice, side by side, on a dense view without position-space sizes (the LDS loop's):
//   side A   mcf_pivot_walk, mcf_pivot_finish, mcf_apply_one              -- what every other path runs;
//   side B   mcf_pivot_walk, mcf_pivot_finish_t<true>, mcf_apply_one_paths -- what the LDS loop runs;
// and holds them against each other at every pivot: the control block after the decision, (source, in_t2, ddepth) of every
// position of [lo, hi) from A's segment table and from B's paths, node records / flows / states / weights after the finish
// pass, and every array after the apply pass.  It is NOT a CPU path of the library: nothing in the package loads it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mcf_host.h"

namespace {

struct Side {
    McfHostImage im;
    std::vector<int32_t> order1, path1, path2, pos1, ppos1, ppos2, chg;
    std::vector<McfNode> rec1, rec2;
    std::vector<McfSeg> seg;
    McfCtx ctx;
    McfView view{};
    McfDevex dx;
};

const McfSeg kUntouched = McfSeg{-7, -7, -7, -7};

void bind(Side& s, int32_t rule, int64_t block_size, int64_t max_pivots) {
    McfHostImage& im = s.im;
    const size_t N = (size_t)im.n_nodes;
    s.order1 = im.order;
    s.pos1 = im.pos;
    s.path1.assign(N, 0); s.path2.assign(N, 0);
    s.ppos1.assign(2 * N, 0); s.ppos2.assign(2 * N, 0);
    s.rec1.assign(N, McfNode{0, 0, 0, 0}); s.rec2.assign(N, McfNode{0, 0, 0, 0});
    s.seg.assign(2 * N + 2, kUntouched);
    s.chg.assign(N, 0);
    std::memset(&s.ctx, 0, sizeof s.ctx);
    std::memset(&s.dx, 0, sizeof s.dx);
    s.ctx.unbounded_arc = -1;
    McfView& v = s.view;
    v.n_nodes = im.n_nodes;
    v.m = im.m;
    v.tail = im.tail.data(); v.head = im.head.data(); v.cost = im.cost.data(); v.orig = im.orig.data();
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) v.bucket_off[x] = im.bucket_off[x];
    v.state = im.state.data();
    v.weight = rule == MCF_RULE_DEVEX_BLOCK ? im.weight.data() : nullptr;
    v.dx = rule == MCF_RULE_DEVEX_BLOCK ? &s.dx : nullptr;
    mcf_devex_fill_granules(&s.dx, im.bucket_off);
    v.arcw = im.arcw.data();
    v.pi = im.pi.data();
    v.node = im.node.data();
    v.order[0] = im.order.data(); v.order[1] = s.order1.data();
    v.path1 = s.path1.data(); v.path2 = s.path2.data();
    v.ppos1 = s.ppos1.data(); v.ppos2 = s.ppos2.data();
    v.rec1 = s.rec1.data(); v.rec2 = s.rec2.data();
    v.seg = s.seg.data();
    v.ctx = &s.ctx;
    v.key_mode = MCF_KEY_PLAIN;
    v.vk_bigm = im.big_m; v.vk_half = 1 << 28;
    v.posbuf[0] = im.pos.data(); v.posbuf[1] = s.pos1.data();
    v.chg = s.chg.data();
    // (psz, reach, the blocked list, resident reduced costs, dirty flags: null -- the dense layout of the LDS loop)
    s.ctx.max_pivots = max_pivots < 0 ? INT64_MAX : max_pivots;
    mcf_init_block_state(&s.ctx, rule, im.m, block_size);
    s.ctx.climb_budget = INT32_MAX;   // always the climb: the view keeps no sizes to scan
    s.ctx.climb_depth = 0;
}

// the pricing sweep of oracle/emul_engine.cpp for one rank: Dantzig over everything, Devex over the current block
void price(const Side& s, int32_t rule, int64_t* key, int64_t* arc, int64_t* priced) {
    const McfView& v = s.view;
    const bool devex = rule == MCF_RULE_DEVEX_BLOCK;
    int64_t bk = 0, ba = -1, np = 0;
    for (int x = 0; x < MCF_NUM_BUCKETS; ++x) {
        int64_t lo, hi;
        if (devex) mcf_devex_slice(v.dx, x, 0, 1, (int32_t)v.ctx->block_index, v.ctx->block_granules, &lo, &hi);
        else mcf_bucket_slice(v.bucket_off, x, 0, 1, 0, 1, &lo, &hi);
        np += hi - lo;
        for (int64_t i = lo; i < hi; ++i) {
            if (!v.state[i]) continue;
            const int64_t viol = mcf_violation(v, i);
            if (viol <= 0) continue;
            int64_t kk = mcf_dantzig_key(v, i, viol, v.state[i]);
            if (devex) {
                const double merit = ((double)viol * (double)viol) / (double)v.weight[i];
                std::memcpy(&kk, &merit, 8);
            }
            const int64_t id = mcf_pack_arc(devex ? mcf_devex_tie_id(v.orig[i], v.state[i]) : v.orig[i], i);
            if (mcf_cand_better(kk, id, bk, ba)) { bk = kk; ba = id; }
        }
    }
    *key = bk; *arc = ba; *priced = np;
}

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// the arrays a finish pass writes
bool same_finished(const Side& a, const Side& b) {
    return same(a.im.node, b.im.node) && same(a.im.arcw, b.im.arcw) && same(a.im.state, b.im.state) && same(a.im.weight, b.im.weight);
}
// ... and everything a pivot leaves behind
bool same_all(const Side& a, const Side& b) {
    return same_finished(a, b) && same(a.im.pi, b.im.pi) && same(a.im.order, b.im.order) && same(a.order1, b.order1) &&
           same(a.im.pos, b.im.pos) && same(a.pos1, b.pos1) && std::memcmp(&a.ctx, &b.ctx, sizeof(McfCtx)) == 0;
}

}  // namespace

extern "C" {

enum {
    AP_PIVOTS = 0, AP_SWAPS, AP_FLIPS, AP_POSITIONS, AP_BAD_SOURCES, AP_BAD_STATES, AP_MAX_K, AP_MULTI_PIECE, AP_BEHIND_VIN,
    AP_END_OF_BLOCK, AP_FIRST_SIDE, AP_SECOND_SIDE, AP_EMPTY_RIGHT, AP_TABLE_WRITTEN, AP_STATUS, AP_FIRST_BAD, AP_MAX_RANGE,
    AP_FIRST_K, AP_REPORT_LEN
};

int32_t mcf_apply_paths_report_len() { return AP_REPORT_LEN; }

// Whole host pivots on both sides (see the head of this file).  Arcs in the caller's order; in_tree / at_upper: a start basis as
// for mcf_set_basis, or null for the cold start.  rule: MCF_RULE_DANTZIG or MCF_RULE_DEVEX_BLOCK.  max_pivots < 0: to the end.
// report[AP_REPORT_LEN]: pivots, basis swaps, bound flips, positions of [lo, hi) compared, positions whose (source, in_t2,
// ddepth) differ, pivots after which the two sides differ in any array or in the control block, greatest stem index of a leaving
// arc, swaps with more than one piece, insertions directly behind v_in, insertions at the end of v_in's block (a v_in without
// descendants counts as behind), swaps with the leaving arc on the first / on the second side, pieces whose right segment is
// empty, pivots after which side B's segment table was no longer untouched, final status (MCF_* of the control block), first
// pivot with a difference (-1: none), widest moved range hi - lo, stem index of the FIRST swap (-1: none).
// flow[m] / pi[n + 1] / parent[n + 1] / depth[n + 1] (each may be null) <- side B's final state, caller's arc order.
// Returns 0, 1 when the basis was refused, -1 on bad arguments, -2 on an internal error of the pivot.
int mcf_apply_paths_run_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                             const int64_t* supply, const int8_t* in_tree, const int8_t* at_upper, int32_t rule, int64_t block_size,
                             int64_t max_pivots, int64_t* report, int64_t* flow, int64_t* pi, int32_t* parent, int32_t* depth) {
    if (!report || (rule != MCF_RULE_DANTZIG && rule != MCF_RULE_DEVEX_BLOCK)) return -1;
    for (int k = 0; k < AP_REPORT_LEN; ++k) report[k] = 0;
    report[AP_FIRST_BAD] = -1; report[AP_FIRST_K] = -1;
    Side A;
    int code = 0;
    const std::string bad = mcf_build_image(n, m, tail, head, cost, cap, supply, A.im, &code);
    if (!bad.empty()) return -1;
    if (in_tree) {
        const std::string msg = mcf_apply_basis(A.im, in_tree, at_upper);
        if (!msg.empty()) return 1;
    }
    Side B;
    B.im = A.im;
    bind(A, rule, block_size, max_pivots);
    bind(B, rule, block_size, max_pivots);
    auto flag = [&](int which) {
        report[which] += 1;
        if (report[AP_FIRST_BAD] < 0) report[AP_FIRST_BAD] = A.ctx.pivots;
    };
    while (A.ctx.status == MCF_RUNNING) {
        int64_t key, arc, priced, keyb, arcb, pricedb;
        price(A, rule, &key, &arc, &priced);
        price(B, rule, &keyb, &arcb, &pricedb);
        if (key != keyb || arc != arcb) { flag(AP_BAD_STATES); break; }
        if (A.ctx.pivots < A.ctx.max_pivots) { A.ctx.arcs_priced += priced; B.ctx.arcs_priced += priced; }
        mcf_pivot_walk(A.view, key, arc, rule);
        mcf_pivot_walk(B.view, key, arc, rule);
        if (std::memcmp(&A.ctx, &B.ctx, sizeof(McfCtx)) != 0) { flag(AP_BAD_STATES); break; }
        if (A.ctx.status == MCF_INTERNAL_ERROR) return -2;
        const McfCtx& c = A.ctx;
        const bool swap = c.stage == 2;
        int32_t vin_size = 0, pvin = 0;
        if (swap) {   // (before the finish pass rewrites sizes)
            vin_size = A.view.node[c.pv_vin].size;
            pvin = (c.cur ? A.view.posbuf[1] : A.view.posbuf[0])[c.pv_vin];
        }
        mcf_pivot_finish(A.view, mcf_view_paths(A.view), 0, 1);
        if (swap) {
            // ---- the sources, position by position: A's table against B's paths (B has not finished yet: nothing it reads is
            // something the finish pass writes)
            const McfNode* srec = c.pv_result == 1 ? B.view.rec1 : B.view.rec2;
            const int32_t* spos = c.pv_result == 1 ? B.view.ppos1 : B.view.ppos2;
            for (int32_t j = c.lo; j < c.hi; ++j) {
                bool ta = false, tb = false;
                int32_t da = 0, db = 0;
                const int32_t ia = mcf_apply_source(A.ctx, A.view.seg, j, &ta, &da);
                const int32_t ib = mcf_apply_source_paths(B.ctx, srec, spos, j, &tb, &db);
                report[AP_POSITIONS] += 1;
                if (ia != ib || ta != tb || da != db) flag(AP_BAD_SOURCES);
            }
            const int32_t k = c.pv_k, S = c.t2_size, a0 = c.t2_old, b = c.t2_new;
            // the insertion point in old coordinates, chosen as mcf_pivot_swap chooses it
            const int32_t tA = pvin + 1, tB = pvin + vin_size;
            const int32_t costA = tA <= a0 ? a0 - tA : tA - (a0 + S), costB = tB <= a0 ? a0 - tB : tB - (a0 + S);
            const int32_t t = costA <= costB ? tA : tB;
            if ((t <= a0 ? t : t - S) != b) flag(AP_BAD_STATES);
            report[AP_SWAPS] += 1;
            if (report[AP_FIRST_K] < 0) report[AP_FIRST_K] = k;
            if (k > report[AP_MAX_K]) report[AP_MAX_K] = k;
            if (k > 0) report[AP_MULTI_PIECE] += 1;
            report[t == tA ? AP_BEHIND_VIN : AP_END_OF_BLOCK] += 1;
            report[c.pv_result == 1 ? AP_FIRST_SIDE : AP_SECOND_SIDE] += 1;
            for (int32_t i = 1; i <= k; ++i)
                if (spos[i] + srec[i].size == spos[i - 1] + srec[i - 1].size) report[AP_EMPTY_RIGHT] += 1;
            if (c.hi - c.lo > report[AP_MAX_RANGE]) report[AP_MAX_RANGE] = c.hi - c.lo;
        } else if (c.stage == 1) {
            report[AP_FLIPS] += 1;
        }
        mcf_pivot_finish_t<true>(B.view, mcf_view_paths(B.view), 0, 1);
        for (const McfSeg& sg : B.seg)
            if (std::memcmp(&sg, &kUntouched, sizeof sg) != 0) { flag(AP_TABLE_WRITTEN); break; }
        if (!same_finished(A, B)) flag(AP_BAD_STATES);
        if (c.apply) {
            const McfNode* srec = B.ctx.pv_result == 1 ? B.view.rec1 : B.view.rec2;
            const int32_t* spos = B.ctx.pv_result == 1 ? B.view.ppos1 : B.view.ppos2;
            for (int32_t j = c.lo; j < c.hi; ++j) { mcf_apply_one(A.view, A.ctx, j); mcf_apply_one_paths(B.view, B.ctx, srec, spos, j); }
            for (int32_t j = c.prev_lo; j < c.prev_hi; ++j)
                if (j < c.lo || j >= c.hi) { mcf_apply_one(A.view, A.ctx, j); mcf_apply_one_paths(B.view, B.ctx, srec, spos, j); }
        }
        if (!same_all(A, B)) flag(AP_BAD_STATES);
    }
    report[AP_PIVOTS] = A.ctx.pivots;
    report[AP_STATUS] = A.ctx.status;
    for (int64_t e = 0; e < m; ++e)
        if (flow) flow[B.im.orig[(size_t)e]] = B.im.arcw[(size_t)e].flow;
    for (int32_t u = 0; u <= n; ++u) {
        if (pi) pi[u] = B.im.pi[(size_t)u];
        if (parent) parent[u] = B.im.node[(size_t)u].parent;
        if (depth) depth[u] = B.im.node[(size_t)u].depth;
    }
    return 0;
}

}  // extern "C"
