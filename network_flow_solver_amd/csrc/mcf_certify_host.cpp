// mcf_certify_host.cpp -- host restatement of the certificate's per-arc / per-node logic, test infrastructure only.
//
// The kernels of mcf_certify (mcf_engine.hip: k_cert_arcs, k_cert_nodes) call the MCF_HD functions of mcf_core.h; this
// file calls the very same functions from plain loops, so the CPU test-suite can hold them against Python-int
// yardsticks and planted violations without a device.  It is NOT a CPU path of the library: nothing in the package
// loads it, and it certifies caller's arrays only (there is no resident state on the host).
//
// Arcs are processed in chunks of 64 with an accumulator each, and the chunks are merged LAST to first: the merge order
// differs from any a device run uses, which is the point -- the result may not depend on it.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcf_core.h"

extern "C" {

// out[24]: negative_flow_count, over_capacity_count, bounds_worst, bounds_worst_arc, imbalance_count, imbalance_worst,
// imbalance_worst_node, dual_lower_count, dual_lower_worst, dual_lower_arc, dual_upper_count, dual_upper_worst,
// dual_upper_arc, primal hi / lo, dual hi / lo, gap hi / lo, saturated_arcs, verdict (0 not proven, 1 optimal), 3 spare.
int mcf_certify_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                     const int64_t* supply, const int64_t* flow, const int64_t* potential, uint32_t checks, int64_t* out) {
    if (n < 1 || m < 0 || !supply || !flow || !potential || !out || (checks & ~MCF_CERT_ALL)) return -1;
    if (!checks) checks = MCF_CERT_ALL;
    checks &= ~(MCF_CERT_BASIS | MCF_CERT_PRICING);
    constexpr int64_t kChunk = 64;
    std::vector<McfCertArcAcc> parts((size_t)((m + kChunk - 1) / kChunk));
    for (size_t c = 0; c < parts.size(); ++c) {
        mcf_cert_arc_init(&parts[c]);
        const int64_t lo = (int64_t)c * kChunk, hi = lo + kChunk < m ? lo + kChunk : m;
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t cp = (cap[i] < 0 || cap[i] >= MCF_INF) ? MCF_INF : cap[i];
            const int64_t rc = cost[i] + potential[tail[i]] - potential[head[i]];
            mcf_cert_arc(&parts[c], checks, i, cost[i], cp, flow[i], rc);
        }
    }
    McfCertArcAcc A;
    mcf_cert_arc_init(&A);
    for (size_t c = parts.size(); c-- > 0;) mcf_cert_arc_merge(&A, parts[c]);

    std::vector<__int128> bal((size_t)n);
    for (int32_t v = 0; v < n; ++v) bal[(size_t)v] = supply[v];
    for (int64_t i = 0; i < m; ++i) { bal[(size_t)tail[i]] -= flow[i]; bal[(size_t)head[i]] += flow[i]; }
    McfCertNodeAcc N;
    mcf_cert_node_init(&N);
    for (int32_t v = n; v-- > 0;) {
        McfCertNodeAcc one;
        mcf_cert_node_init(&one);
        if (checks & MCF_CERT_CONSERVATION) mcf_cert_node_balance(&one, v, bal[(size_t)v]);
        if (checks & MCF_CERT_OBJECTIVES) mcf_cert_add128(&one.dnode_lo, &one.dnode_hi, (mcf_u128)(-(__int128)potential[v] * supply[v]));
        mcf_cert_node_merge(&N, one);
    }
    auto idx = [](int64_t i) { return i == MCF_CERT_NONE ? (int64_t)-1 : i; };
    const __int128 primal = (__int128)(((mcf_u128)A.primal_hi << 64) | A.primal_lo);
    const __int128 dual = (__int128)((((mcf_u128)N.dnode_hi << 64) | N.dnode_lo) + (((mcf_u128)A.dcap_hi << 64) | A.dcap_lo));
    const __int128 gap = primal - dual;
    std::memset(out, 0, 24 * sizeof(int64_t));
    out[0] = A.neg_n; out[1] = A.over_n; out[2] = A.bnd_w; out[3] = idx(A.bnd_i);
    out[4] = N.imb_n; out[5] = N.imb_w; out[6] = idx(N.imb_i);
    out[7] = A.dlo_n; out[8] = A.dlo_w; out[9] = idx(A.dlo_i);
    out[10] = A.dup_n; out[11] = A.dup_w; out[12] = idx(A.dup_i);
    out[13] = (int64_t)(primal >> 64); out[14] = (int64_t)(uint64_t)primal;
    out[15] = (int64_t)(dual >> 64); out[16] = (int64_t)(uint64_t)dual;
    out[17] = (int64_t)(gap >> 64); out[18] = (int64_t)(uint64_t)gap;
    out[19] = A.sat_n;
    const uint32_t need = MCF_CERT_BOUNDS | MCF_CERT_CONSERVATION | MCF_CERT_DUAL | MCF_CERT_OBJECTIVES;
    out[20] = ((checks & need) == need && !A.neg_n && !A.over_n && !N.imb_n && !A.dlo_n && !A.dup_n && gap == 0) ? 1 : 0;
    return 0;
}

// the bottleneck predicate of mcf_bottlenecks over caller's arrays; indices ascending; returns the count
int64_t mcf_bottlenecks_host(int64_t m, const int64_t* cap, const int64_t* flow, int64_t num, int64_t den, int64_t* idx_out, int64_t idx_cap) {
    int64_t count = 0;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t cp = (cap[i] < 0 || cap[i] >= MCF_INF) ? MCF_INF : cap[i];
        if (!mcf_cert_bottleneck(cp, flow[i], num, den)) continue;
        if (count < idx_cap) idx_out[count] = i;
        ++count;
    }
    return count;
}

}  // extern "C"
