// mcf_small_budget_host.cpp -- host restatement of what the fused LDS loop's 256-lane front kernel changed in the second part of
// its slot budget, test infrastructure only.
//
// * Pairs.  mcf_small_plan (mcf_core.h) lays the arrays of a side or of a buffer a constant distance apart, and the kernel names
//   "the second one's element i" as the first one's element i + bit * distance (mcf_pair_bit, mcf_pair_index) where it selected
//   between two base addresses.  mcf_budget_pairs_host plans an instance and holds the two forms against each other for every
//   index of both sides and both buffers, the search's merged index included, and checks the alignment of every record address.
// * Counts.  A wave files its two counts of one-sided ancestors as one word (mcf_counts_pack); a reader adds the waves' words and
//   unpacks.  mcf_budget_counts_host does that for four waves.
// * Whole pivots.  mcf_budget_twin_host runs whole host solves twice, side by side: side A as every other path runs a pivot
//   (mcf_pivot_walk, mcf_pivot_finish_t<true>, mcf_apply_one_paths on separate arrays), side B as the kernel runs it -- ONE buffer
//   laid out by mcf_small_plan, mcf_pivot_decide_flat_t<true>, mcf_pivot_finish_pairs and the apply pass with its three buffers
//   and the leaving side named by pair arithmetic -- and compares the control block after every decision and every array after
//   every pivot.
// It is NOT a CPU path of the library: nothing in the package loads it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mcf_host.h"

namespace {

template <typename T> T* at(std::vector<unsigned char>& buf, uint32_t off) { return reinterpret_cast<T*>(buf.data() + off); }

template <typename T>
bool same(const std::vector<T>& a, const T* b) { return a.empty() || std::memcmp(a.data(), b, a.size() * sizeof(T)) == 0; }

struct Twin {
    McfHostImage im;       // side A's arrays (and both sides' arc constants)
    std::vector<int32_t> order1, pos1, path1, path2, ppos1, ppos2;
    std::vector<McfNode> rec1, rec2;
    std::vector<McfSeg> seg;
    McfCtx ctx_a, ctx_b;
    McfView a{}, b{};
    McfSmallLayout L;
    std::vector<unsigned char> buf;   // side B: the LDS image
};

void bind_common(McfView& v, const McfHostImage& im, McfCtx* ctx, int64_t max_pivots) {
    v.n_nodes = im.n_nodes;
    v.m = im.m;
    v.tail = im.tail.data(); v.head = im.head.data(); v.cost = im.cost.data(); v.orig = im.orig.data();
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) v.bucket_off[x] = im.bucket_off[x];
    v.key_mode = MCF_KEY_PLAIN;
    v.vk_bigm = im.big_m; v.vk_half = 1 << 28;
    std::memset(ctx, 0, sizeof *ctx);
    ctx->unbounded_arc = -1;
    ctx->max_pivots = max_pivots < 0 ? INT64_MAX : max_pivots;
    mcf_init_block_state(ctx, MCF_RULE_DANTZIG, im.m, 0);
    ctx->climb_budget = INT32_MAX;   // always the climb: the view keeps no sizes to scan
    ctx->climb_depth = 0;
    v.ctx = ctx;
}

bool bind(Twin& t, int64_t max_pivots) {
    McfHostImage& im = t.im;
    const size_t N = (size_t)im.n_nodes;
    if (!mcf_small_plan(im.m_pad, (uint64_t)im.arcw.size(), im.n_nodes, false, &t.L)) return false;
    t.order1 = im.order; t.pos1 = im.pos;
    t.path1.assign(N, 0); t.path2.assign(N, 0); t.ppos1.assign(N, 0); t.ppos2.assign(N, 0);
    t.rec1.assign(N, McfNode{0, 0, 0, 0}); t.rec2.assign(N, McfNode{0, 0, 0, 0});
    t.seg.assign(2 * N + 2, McfSeg{0, 0, 0, 0});
    t.buf.assign(t.L.total, 0xa5);   // (whatever an earlier launch left in LDS)
    const McfSmallLayout& L = t.L;
    std::memcpy(at<int8_t>(t.buf, L.state), im.state.data(), im.state.size());
    std::memcpy(at<McfArcW>(t.buf, L.arcw), im.arcw.data(), im.arcw.size() * sizeof(McfArcW));
    std::memcpy(at<int64_t>(t.buf, L.pi), im.pi.data(), N * 8);
    std::memcpy(at<McfNode>(t.buf, L.node), im.node.data(), N * 16);
    std::memcpy(at<int32_t>(t.buf, L.order0), im.order.data(), N * 4);
    std::memcpy(at<int32_t>(t.buf, L.order1), im.order.data(), N * 4);
    std::memcpy(at<int32_t>(t.buf, L.pos0), im.pos.data(), N * 4);
    std::memcpy(at<int32_t>(t.buf, L.pos1), im.pos.data(), N * 4);
    bind_common(t.a, im, &t.ctx_a, max_pivots);
    bind_common(t.b, im, &t.ctx_b, max_pivots);
    McfView& a = t.a;
    a.state = im.state.data(); a.arcw = im.arcw.data(); a.pi = im.pi.data(); a.node = im.node.data();
    a.order[0] = im.order.data(); a.order[1] = t.order1.data(); a.posbuf[0] = im.pos.data(); a.posbuf[1] = t.pos1.data();
    a.path1 = t.path1.data(); a.path2 = t.path2.data(); a.ppos1 = t.ppos1.data(); a.ppos2 = t.ppos2.data();
    a.rec1 = t.rec1.data(); a.rec2 = t.rec2.data(); a.seg = t.seg.data();
    McfView& b = t.b;   // (small_map_view)
    b.state = at<int8_t>(t.buf, L.state); b.arcw = at<McfArcW>(t.buf, L.arcw); b.pi = at<int64_t>(t.buf, L.pi); b.node = at<McfNode>(t.buf, L.node);
    b.order[0] = at<int32_t>(t.buf, L.order0); b.order[1] = at<int32_t>(t.buf, L.order1);
    b.posbuf[0] = at<int32_t>(t.buf, L.pos0); b.posbuf[1] = at<int32_t>(t.buf, L.pos1);
    b.path1 = at<int32_t>(t.buf, L.path1); b.path2 = at<int32_t>(t.buf, L.path2);
    b.ppos1 = at<int32_t>(t.buf, L.ppos1); b.ppos2 = at<int32_t>(t.buf, L.ppos2);
    b.rec1 = at<McfNode>(t.buf, L.rec1); b.rec2 = at<McfNode>(t.buf, L.rec2); b.seg = at<McfSeg>(t.buf, L.seg);
    return true;
}

// Dantzig over everything, as oracle/emul_engine.cpp prices for one rank
void price(const McfView& v, int64_t* key, int64_t* arc, int64_t* priced) {
    int64_t bk = 0, ba = -1, np = 0;
    for (int x = 0; x < MCF_NUM_BUCKETS; ++x) {
        int64_t lo, hi;
        mcf_bucket_slice(v.bucket_off, x, 0, 1, 0, 1, &lo, &hi);
        np += hi - lo;
        for (int64_t i = lo; i < hi; ++i) {
            if (!v.state[i]) continue;
            const int64_t viol = mcf_violation(v, i);
            if (viol <= 0) continue;
            const int64_t id = mcf_pack_arc(v.orig[i], i);
            if (mcf_cand_better(viol, id, bk, ba)) { bk = viol; ba = id; }
        }
    }
    *key = bk; *arc = ba; *priced = np;
}

bool same_arrays(const Twin& t) {
    const McfHostImage& im = t.im;
    const McfView& b = t.b;
    return same(im.state, b.state) && same(im.arcw, b.arcw) && same(im.pi, b.pi) && same(im.node, b.node) && same(im.order, b.order[0]) &&
           same(t.order1, b.order[1]) && same(im.pos, b.posbuf[0]) && same(t.pos1, b.posbuf[1]);
}

}  // namespace

extern "C" {

// Lays out an instance of n_nodes tree nodes and m_pad padded arcs (arcw_count arc records) and compares, for both sides / buffers
// and every index i < n_nodes, the byte offset "base of the selected array + i * size" with "base of the first array +
// mcf_pair_index(i, bit, distance) * size": order, pos, path, ppos (4 bytes), rec (16), the search's residuals (8, in the
// scratch).  Then the search's merged index for every pair of end-point depths below `depths` and every node depth not above
// them: (au ? du0 : dw0) - depth into the selected array against mcf_pair_index(du0 - depth, bit, dw0 - du0 + distance) into the
// first.  out[0]: addresses compared, out[1]: mismatches, out[2]: rec addresses not 16-byte aligned, out[3]: L.total,
// out[4]: the 4-byte distance in elements, out[5]: the 16-byte one, out[6]: 1 when mcf_small_plan accepts the instance (the
// offsets are mcf_small_layout's either way: the plan's bound on tree nodes is reached by no instance with arcs).
int mcf_budget_pairs_host(int32_t n_nodes, int64_t m_pad, int64_t arcw_count, int32_t devex, int32_t depths, int64_t* out) {
    if (!out || n_nodes < 2 || m_pad < 0 || arcw_count < 0) return -1;
    for (int i = 0; i < 7; ++i) out[i] = 0;
    const McfSmallLayout L = mcf_small_layout(m_pad, (uint64_t)arcw_count, n_nodes, devex != 0);
    McfSmallLayout planned;
    if (mcf_small_plan(m_pad, (uint64_t)arcw_count, n_nodes, devex != 0, &planned)) {
        if (std::memcmp(&planned, &L, sizeof L) != 0) return -2;
        out[6] = 1;
    }
    const int32_t d4 = mcf_pair_dist4(n_nodes), d16 = mcf_pair_dist16(n_nodes);
    out[3] = L.total; out[4] = d4; out[5] = d16;
    const uint32_t four[4][2] = {{L.order0, L.order1}, {L.pos0, L.pos1}, {L.path1, L.path2}, {L.ppos1, L.ppos2}};
    auto cmp = [&](uint32_t select_form, uint32_t pair_form) { out[0] += 1; if (select_form != pair_form) out[1] += 1; };
    for (int second = 0; second < 2; ++second) {
        const int32_t bit = mcf_pair_bit(second != 0);
        for (int32_t i = 0; i < n_nodes; ++i) {
            for (const auto& p : four) cmp(p[second] + 4u * (uint32_t)i, p[0] + 4u * (uint32_t)mcf_pair_index(i, bit, d4));
            const uint32_t rec = L.rec1 + 16u * (uint32_t)mcf_pair_index(i, bit, d16);
            cmp((second ? L.rec2 : L.rec1) + 16u * (uint32_t)i, rec);
            if (rec & 15u) out[2] += 1;
            if (n_nodes <= MCF_SMALL_CYCLE_MAX_NODES)   // (res2 = res1 + n_nodes)
                cmp(L.scratch + 8u * (uint32_t)((second ? n_nodes : 0) + i), L.scratch + 8u * (uint32_t)mcf_pair_index(i, bit, d16));
        }
        const int32_t top = depths < n_nodes ? depths : n_nodes;
        for (int32_t du0 = 0; du0 < top; ++du0) for (int32_t dw0 = 0; dw0 < top; ++dw0) {
            const int32_t dend = second ? dw0 : du0;
            for (int32_t depth = 0; depth <= dend; ++depth) {
                const int32_t idx = dend - depth;
                cmp((second ? L.path2 : L.path1) + 4u * (uint32_t)idx, L.path1 + 4u * (uint32_t)mcf_pair_index(du0 - depth, bit, dw0 - du0 + d4));
                const uint32_t rec = L.rec1 + 16u * (uint32_t)mcf_pair_index(du0 - depth, bit, dw0 - du0 + d16);
                cmp((second ? L.rec2 : L.rec1) + 16u * (uint32_t)idx, rec);
                if (rec & 15u) out[2] += 1;
            }
        }
    }
    return 0;
}

// Four waves' counts packed, added and unpacked.  Returns 0 when the sums are n1[0] + .. + n1[3] and n2[0] + .. + n2[3].
int mcf_budget_counts_host(const int32_t* n1, const int32_t* n2, int32_t* sum1, int32_t* sum2) {
    if (!n1 || !n2 || !sum1 || !sum2) return -1;
    uint32_t sum = 0;
    int32_t w1 = 0, w2 = 0;
    for (int q = 0; q < 4; ++q) {
        if (n1[q] < 0 || n2[q] < 0) return -1;
        sum += mcf_counts_pack(n1[q], n2[q]);
        w1 += n1[q]; w2 += n2[q];
    }
    *sum1 = mcf_counts_first(sum); *sum2 = mcf_counts_second(sum);
    return (*sum1 == w1 && *sum2 == w2) ? 0 : 1;
}
int32_t mcf_budget_max_nodes_host(void) { return MCF_SMALL_MAX_NODES; }

// Whole host pivots on both sides (see the head of this file), Dantzig's rule, from the cold start.  max_pivots < 0: to the end.
// report[12] ([10], [11]: swaps with the leaving arc on the first / second side while cur == 1): pivots, basis swaps, bound flips, swaps with the leaving arc on the first side, on the second, pivots with cur == 1
// at the swap, pivots after which the control blocks differ, pivots after which an array differs, final status, first pivot
// with a difference (-1: none).  Returns 0, 1 when the instance does not fit the LDS plan, -1 on bad arguments, -2 on an
// internal error of the pivot.
int mcf_budget_twin_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                         const int64_t* supply, int64_t max_pivots, int32_t finish_mode, int64_t* report) {
    if (!report || finish_mode < 0 || finish_mode > 2) return -1;
    for (int k = 0; k < 12; ++k) report[k] = 0;
    report[9] = -1;
    Twin t;
    int code = 0;
    if (!mcf_build_image(n, m, tail, head, cost, cap, supply, t.im, &code).empty()) return -1;
    if (!bind(t, max_pivots)) return 1;
    const int32_t d4 = mcf_pair_dist4(t.im.n_nodes), d16 = mcf_pair_dist16(t.im.n_nodes);
    McfCtx &ca = t.ctx_a, &cb = t.ctx_b;
    auto flag = [&](int which) { report[which] += 1; if (report[9] < 0) report[9] = ca.pivots; };
    while (ca.status == MCF_RUNNING) {
        int64_t key, arc, priced, keyb, arcb, pricedb;
        price(t.a, &key, &arc, &priced);
        price(t.b, &keyb, &arcb, &pricedb);
        if (key != keyb || arc != arcb) { flag(7); break; }
        if (ca.pivots < ca.max_pivots) { ca.arcs_priced += priced; cb.arcs_priced += priced; }
        mcf_pivot_walk(t.a, key, arc, MCF_RULE_DANTZIG);
        // side B: begin, the climb into the planned path arrays, the flat decide with the leaving node fetched by pair arithmetic
        if (mcf_pivot_begin(t.b, key, arc, MCF_RULE_DANTZIG)) {
            McfCycle cy;
            mcf_cycle_init(t.b, &cy);
            if (!mcf_pivot_climb(t.b, mcf_view_paths(t.b), &cy, mcf_climb_budget(t.b, cy)) || cy.u != cy.w) return -2;
            mcf_pivot_decide_flat_t<true>(t.b, mcf_view_paths(t.b), cy, d4, d16);
        }
        if (std::memcmp(&ca, &cb, sizeof(McfCtx)) != 0) { flag(6); break; }
        if (ca.status == MCF_INTERNAL_ERROR) return -2;
        if (ca.stage == 2) {
            report[1] += 1;
            report[ca.pv_result == 1 ? 3 : 4] += 1;
            if (ca.cur) report[5] += 1;
            if (ca.cur) report[ca.pv_result == 1 ? 10 : 11] += 1;
        } else if (ca.stage == 1) {
            report[2] += 1;
        }
        mcf_pivot_finish_t<true>(t.a, mcf_view_paths(t.a), 0, 1);
        // finish_mode 0: one lane, all loads of the first trip together; 1: 64 lanes one after the other, as the finishing wave's
        // lanes (each lane's loads, then its stores); 2: 64 lanes, pass by pass (the trait switched off)
        if (finish_mode == 0) mcf_pivot_finish_pairs<true>(t.b, mcf_view_paths(t.b), d4, d16, 0, 1);
        else for (int32_t lane = 0; lane < 64; ++lane) {
            if (finish_mode == 1) mcf_pivot_finish_pairs<true>(t.b, mcf_view_paths(t.b), d4, d16, lane, 64);
            else mcf_pivot_finish_pairs<false>(t.b, mcf_view_paths(t.b), d4, d16, lane, 64);
        }
        if (ca.apply) {
            const McfNode* sa = ca.pv_result == 1 ? t.a.rec1 : t.a.rec2;
            const int32_t* pa = ca.pv_result == 1 ? t.a.ppos1 : t.a.ppos2;
            // (small_apply: the leaving side and the buffers as numbers)
            const int32_t sbit = cb.pv_result - 1, nbit = cb.cur ^ 1;
            const McfNode* sb = t.b.rec1 + mcf_pair_index(0, sbit, d16);
            const int32_t* pb = t.b.ppos1 + mcf_pair_index(0, sbit, d4);
            const int32_t* src = t.b.order[0] + mcf_pair_index(0, cb.cur, d4);
            int32_t* dst = t.b.order[0] + mcf_pair_index(0, nbit, d4);
            int32_t* pnext = t.b.posbuf[0] + mcf_pair_index(0, nbit, d4);
            for (int32_t j = ca.lo; j < ca.hi; ++j) { mcf_apply_one_paths(t.a, ca, sa, pa, j); mcf_apply_one_paths_at(t.b, cb, sb, pb, src, dst, pnext, j); }
            for (int32_t j = ca.prev_lo; j < ca.prev_hi; ++j)
                if (j < ca.lo || j >= ca.hi) { mcf_apply_one_paths(t.a, ca, sa, pa, j); mcf_apply_one_paths_at(t.b, cb, sb, pb, src, dst, pnext, j); }
        }
        if (std::memcmp(&ca, &cb, sizeof(McfCtx)) != 0) flag(6);
        if (!same_arrays(t)) flag(7);
    }
    report[0] = ca.pivots;
    report[8] = ca.status;
    return 0;
}

}  // extern "C"
