// mcf_ranges_host.cpp -- host restatement of the per-arc / per-node logic of mcf_cost_ranges, test infrastructure only.
//
// The kernels of mcf_cost_ranges (mcf_passes_dev.h: k_rng_*) call the MCF_HD functions of mcf_core.h (mcf_rng_*); this file
// calls the very same functions from plain loops, so the CPU test-suite can hold them against numpy yardsticks on planted
// trees without a device.  It is NOT a CPU path of the library: nothing in the package loads it, and it ranges caller's
// arrays only (there is no resident state on the host).
//
// The merge order differs from any a device run uses, on purpose -- the result may not depend on it: the arcs are walked in
// chunks of `chunk` from the LAST chunk to the first, and every level is pushed from a copy, nodes last to first.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcf_core.h"

extern "C" {

// Arcs in the caller's order; node arrays have n + 1 entries, the root is node n (its parent may be anything outside
// [0, n]; a top of a component may name n or anything outside [0, n) as its parent).  pred_arc[v]: the caller's index of v's
// tree arc, >= m for an artificial one (mcf_get_tree's layout).  down[m], up[m]; report[8]: basic_real, basic_artificial,
// eligible, max_depth, levels, inf_down, inf_up, 0.
int mcf_cost_ranges_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int8_t* state,
                         const int32_t* parent, const int32_t* pred_arc, const int32_t* depth, const int64_t* pi, int64_t chunk,
                         int64_t* down, int64_t* up, int64_t* report) {
    if (n < 1 || m < 0 || !parent || !pred_arc || !depth || !pi || !report || (m > 0 && (!tail || !head || !cost || !state || !down || !up))) return -1;
    if (chunk < 1) chunk = 1;
    const int32_t N = n + 1, root = n;
    std::memset(report, 0, 8 * sizeof(int64_t));
    int64_t max_depth = 0;
    for (int32_t v = 0; v < n; ++v) if (depth[v] > max_depth) max_depth = depth[v];
    const int K = mcf_rng_levels(max_depth);
    report[3] = max_depth; report[4] = K;
    std::vector<int32_t> anc((size_t)K * N);
    std::vector<int64_t> tab[2];   // 0 = P, 1 = N
    tab[0].assign((size_t)K * N, MCF_RNG_INF);
    tab[1].assign((size_t)K * N, MCF_RNG_INF);
    for (int32_t v = 0; v < N; ++v) anc[(size_t)v] = (v == root || parent[v] < 0 || parent[v] >= N) ? root : parent[v];
    for (int k = 1; k < K; ++k)
        for (int32_t v = N; v-- > 0;) anc[(size_t)k * N + v] = anc[(size_t)(k - 1) * N + anc[(size_t)(k - 1) * N + v]];
    auto up_k = [&](int k, int32_t x) { return anc[(size_t)k * N + x]; };

    const int64_t chunks = (m + chunk - 1) / chunk;
    for (int64_t c = chunks; c-- > 0;) {
        const int64_t lo = c * chunk, hi = lo + chunk < m ? lo + chunk : m;
        for (int64_t f = lo; f < hi; ++f) {
            const int32_t st = state[f];
            if (st == 0) continue;
            const int32_t t = tail[f], hd = head[f];
            const int64_t s = mcf_rng_slack(st, cost[f] + pi[t] - pi[hd]);
            if (s < 0) ++report[2];
            mcf_rng_nonbasic(st, s, &down[f], &up[f]);
            mcf_rng_jumps(t, depth[t], hd, depth[hd], K, up_k, [&](int side, int k, int32_t x) {
                mcf_rng_lower(&tab[mcf_rng_table(st, side == 0)][(size_t)k * N + x], s);
            });
        }
    }
    for (int k = K - 1; k >= 1; --k)
        for (int w = 0; w < 2; ++w) {
            const std::vector<int64_t> from(tab[w].begin() + (size_t)k * N, tab[w].begin() + (size_t)(k + 1) * N);
            int64_t* to = tab[w].data() + (size_t)(k - 1) * N;
            for (int32_t x = N; x-- > 0;) mcf_rng_push(from[(size_t)x], &to[x], &to[up_k(k - 1, x)]);
        }
    for (int32_t v = n; v-- > 0;) {
        const int64_t e = pred_arc[v];
        if (e < 0) continue;
        if (e >= m) { ++report[1]; continue; }
        ++report[0];
        mcf_rng_basic(tail[e] == v, tab[0][(size_t)v], tab[1][(size_t)v], &down[e], &up[e]);
    }
    for (int64_t f = 0; f < m; ++f) { if (down[f] == MCF_RNG_INF) ++report[5]; if (up[f] == MCF_RNG_INF) ++report[6]; }
    return 0;
}

}  // extern "C"
