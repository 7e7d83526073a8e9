// mcf_farkas_host.cpp -- host restatement of the per-arc / per-node logic of mcf_certify_ray and mcf_certify_cut, test
// infrastructure only.
//
// The kernels (mcf_engine.hip: k_ray_nodes, k_cut_round, k_cut_arcs, k_cut_nodes) call the MCF_HD functions of mcf_core.h;
// this file calls the very same functions from plain loops over the caller's arrays, so the CPU test-suite can hold them
// against Python-int yardsticks without a device.  It is NOT a CPU path of the library: nothing in the package loads it.
//
// Items are processed in chunks of `chunk` with an accumulator each, and the chunks are merged LAST to first: the merge
// order differs from any a device run uses, and differs between chunk sizes, which is the point -- the result may not
// depend on it.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcf_core.h"

namespace {
inline int64_t capped(int64_t cap) { return (cap < 0 || cap >= MCF_INF) ? MCF_INF : cap; }
inline void put128(int64_t* hi_lo, __int128 x) { hi_lo[0] = (int64_t)(x >> 64); hi_lo[1] = (int64_t)(uint64_t)x; }
}  // namespace

extern "C" {

// The cycle of the non-basic arc `arc`, pushed backward when `backward`, from the tree as mcf_get_tree returns it: parent /
// pred_arc (caller's arc numbers, m + v for the artificial arc of v) / pos / size / depth, n + 1 entries each, and pi[n + 1]
// with the root (node n).  An artificial arc points node -> root when pi[node] < pi[root] (its reduced cost is 0); art[n]
// (may be NULL: zeros) is the flow of every node's artificial arc, signed as in mcf_cut_host.
// out[12]: the int64 fields of mcf_ray in their order; idx_out as there.
int mcf_ray_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap, const int64_t* flow,
                 const int32_t* parent, const int32_t* pred_arc, const int32_t* pos, const int32_t* size, const int32_t* depth,
                 const int64_t* pi, const int64_t* art, int64_t big_m, int64_t arc, int32_t backward, int64_t chunk, int64_t* idx_out, int64_t idx_cap, int64_t* out) {
    if (n < 1 || arc < 0 || arc >= m || chunk < 1 || !out || idx_cap < 0 || (idx_cap > 0 && !idx_out)) return -1;
    const int32_t N = n + 1;
    const int32_t t = tail[arc], hd = head[arc];
    const int32_t first = backward ? t : hd, second = backward ? hd : t;
    std::vector<McfRayAcc> parts((size_t)((N + chunk - 1) / chunk));
    std::vector<int8_t> side((size_t)N, 0);
    for (size_t c = 0; c < parts.size(); ++c) {
        mcf_ray_init(&parts[c]);
        const int64_t lo = (int64_t)c * chunk, hi = lo + chunk < N ? lo + chunk : N;
        for (int64_t u = lo; u < hi; ++u) {
            const int sd = mcf_ray_side(pos[u], size[u], pos[first], pos[second]);
            side[(size_t)u] = (int8_t)sd;
            if (sd == 3) mcf_cert_worst(&parts[c].join_d, &parts[c].join_i, (int64_t)depth[u] + 1, u);
            else if (sd && pred_arc[u] >= 0) {
                const int64_t a = pred_arc[u];
                if (a < m) {
                    const bool up = tail[a] == u && head[a] == parent[u];
                    mcf_ray_arc(&parts[c], a, true, false, sd == 1 ? up : !up, cost[a], capped(cap[a]), flow[a]);
                } else {
                    const bool up = pi[u] < pi[n];
                    const int64_t af = art ? (art[u] < 0 ? -art[u] : art[u]) : 0;
                    mcf_ray_arc(&parts[c], a, true, true, sd == 1 ? up : !up, big_m, MCF_INF, af);
                }
            }
        }
    }
    McfRayAcc R;
    mcf_ray_init(&R);
    for (size_t c = parts.size(); c-- > 0;) mcf_ray_merge(&R, parts[c]);
    McfRayAcc own;
    mcf_ray_init(&own);
    mcf_ray_arc(&own, arc, false, false, !backward, cost[arc], capped(cap[arc]), flow[arc]);
    const int64_t rc = cost[arc] + pi[t] - pi[hd];
    own.rc = backward ? -rc : rc;
    mcf_ray_merge(&R, own);
    const int64_t length = R.tree_n + 1;
    if (idx_cap > 0) idx_out[0] = arc;
    for (int32_t u = 0; u < N; ++u) {
        if ((side[(size_t)u] != 1 && side[(size_t)u] != 2) || pred_arc[u] < 0) continue;
        const int64_t at = side[(size_t)u] == 1 ? 1 + (int64_t)depth[first] - depth[u] : length - 1 - ((int64_t)depth[second] - depth[u]);
        if (at >= 1 && at < idx_cap && at < length) idx_out[at] = pred_arc[u];
    }
    out[0] = arc; out[1] = backward ? 1 : 0; out[2] = length; out[3] = R.join_i == MCF_CERT_NONE ? -1 : R.join_i;
    out[4] = R.back_n; out[5] = R.cap_n; out[6] = R.art_n; out[7] = R.cost; out[8] = R.rc;
    out[9] = R.theta; out[10] = R.theta_i == MCF_CERT_NONE ? -1 : R.theta_i;
    out[11] = mcf_ray_proven(R, backward != 0) ? 1 : 0;
    return 0;
}

// The cut of mcf_certify_cut over the caller's arrays.  in_S == NULL: S is searched from the seeds over flow[m] (caller's
// order) and art[n] (the flow of every node's artificial arc, > 0 towards the root, < 0 from it), level by level as the
// device does, every level by one sweep over the arcs in chunks, last chunk first.  in_S != NULL: the caller's set; flow and
// art may be NULL.  S_out[n] may be NULL.
// out[17]: seeds, nodes_in_S, rounds, deficit_in_S, leaving_arcs, leaving_uncapacitated, leaving_unsaturated,
// entering_with_flow, capacity hi / lo, supply hi / lo, excess hi / lo, artificial_out hi / lo, proven.
int mcf_cut_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cap, const int64_t* supply,
                 const int64_t* flow, const int64_t* art, const int8_t* in_S, int64_t chunk, int8_t* S_out, int64_t* out) {
    if (n < 1 || m < 0 || chunk < 1 || !supply || !out || (!in_S && (!flow || !art))) return -1;
    std::vector<int32_t> mark((size_t)n, 0);
    const int64_t chunks = (m + chunk - 1) / chunk;
    int32_t level = 0;
    if (in_S) {
        for (int32_t v = 0; v < n; ++v) mark[(size_t)v] = in_S[v] ? 1 : 0;
    } else {
        for (int32_t v = 0; v < n; ++v) if (art[v] > 0) { mark[(size_t)v] = 1; level = 1; }
        for (int32_t r = 1; level > 0 && r <= n; ++r) {   // bounded by n rounds, as on the device
            for (int64_t c = chunks; c-- > 0;) {
                const int64_t lo = c * chunk, hi = lo + chunk < m ? lo + chunk : m;
                for (int64_t i = lo; i < hi; ++i) {
                    const int32_t t = tail[i], hd = head[i];
                    if (mark[(size_t)t] == r && mark[(size_t)hd] == 0 && mcf_cut_extends(true, capped(cap[i]), flow[i])) { mark[(size_t)hd] = r + 1; level = r + 1; }
                    if (mark[(size_t)hd] == r && mark[(size_t)t] == 0 && mcf_cut_extends(false, capped(cap[i]), flow[i])) { mark[(size_t)t] = r + 1; level = r + 1; }
                }
            }
            if (level <= r) break;
        }
    }
    const bool resident = in_S == nullptr;
    std::vector<McfCutAcc> parts((size_t)chunks);
    for (int64_t c = 0; c < chunks; ++c) {
        mcf_cut_init(&parts[(size_t)c]);
        const int64_t lo = c * chunk, hi = lo + chunk < m ? lo + chunk : m;
        for (int64_t i = lo; i < hi; ++i)
            mcf_cut_arc(&parts[(size_t)c], mark[(size_t)tail[i]] != 0, mark[(size_t)head[i]] != 0, capped(cap[i]), flow ? flow[i] : 0, resident);
    }
    McfCutAcc C;
    mcf_cut_init(&C);
    for (size_t c = parts.size(); c-- > 0;) mcf_cut_merge(&C, parts[c]);
    for (int32_t v = n; v-- > 0;) {
        if (!mark[(size_t)v]) continue;
        McfCutAcc one;
        mcf_cut_init(&one);
        mcf_cut_node(&one, supply[v], resident ? art[v] : 0);
        mcf_cut_merge(&C, one);
    }
    if (S_out) for (int32_t v = 0; v < n; ++v) S_out[v] = mark[(size_t)v] ? 1 : 0;
    __int128 excess = 0;
    const bool proven = mcf_cut_proven(C, &excess);
    out[0] = C.seeds; out[1] = C.in_s; out[2] = level; out[3] = C.deficit;
    out[4] = C.leave_n; out[5] = C.leave_uncap; out[6] = C.leave_unsat; out[7] = C.enter_flow;
    put128(out + 8, (__int128)(((mcf_u128)C.cap_hi << 64) | C.cap_lo));
    put128(out + 10, (__int128)(((mcf_u128)C.sup_hi << 64) | C.sup_lo));
    put128(out + 12, excess);
    put128(out + 14, (__int128)(((mcf_u128)C.art_hi << 64) | C.art_lo));
    out[16] = proven ? 1 : 0;
    return 0;
}

}  // extern "C"
