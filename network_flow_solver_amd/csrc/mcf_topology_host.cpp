// mcf_topology_host.cpp -- host restatement of the index arithmetic of mcf_add_arcs, test infrastructure only.
//
// The kernels (mcf_passes_dev.h: k_aa_*) call the MCF_HD functions mcf_topo_* of mcf_core.h; this file calls the very same
// functions from plain loops, so the CPU test-suite can hold the merged layout against mcf_build_image of the extended
// instance without a device.  It is NOT a CPU path of the library: nothing in the package loads it.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "mcf_host.h"

namespace {
int build(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, McfHostImage& im) {
    std::vector<int64_t> zero_arc((size_t)(m > 0 ? m : 1), 0), zero_node((size_t)n, 0);
    int err = 0;
    const std::string msg = mcf_build_image(n, m, tail, head, zero_arc.data(), zero_arc.data(), zero_node.data(), im, &err);
    if (err) return err;
    mcf_build_rcache(im);
    return 0;
}
void put(const McfHostImage& im, int32_t* orig, int32_t* tail, int32_t* head, int64_t* bucket_off, int64_t* adj_off, int64_t* adj) {
    for (int64_t e = 0; e < im.m; ++e) { orig[e] = im.orig[(size_t)e]; tail[e] = im.tail[(size_t)e]; head[e] = im.head[(size_t)e]; }
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) bucket_off[x] = im.bucket_off[x];
    for (int32_t u = 0; u <= im.n; ++u) adj_off[u] = im.adj_off[(size_t)u];
    for (size_t p = 0; p < im.adj.size(); ++p) adj[p] = im.adj[p];
}
}  // namespace

extern "C" {

// Engine order of an instance as mcf_create lays it out: orig / tail / head [m], bucket_off [9], adj_off [n + 1], adj [2m].
int mcf_topology_image_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, int32_t* orig_out, int32_t* tail_out,
                            int32_t* head_out, int64_t* bucket_off_out, int64_t* adj_off_out, int64_t* adj_out) {
    McfHostImage im;
    const int rc = build(n, m, tail, head, im);
    if (rc) return rc;
    put(im, orig_out, tail_out, head_out, bucket_off_out, adj_off_out, adj_out);
    return 0;
}

// The image of the base instance merged with k new arcs by the counting rules of mcf_core.h, one arc / node / adjacency entry
// at a time as the kernels do it: outputs sized for m + k arcs.  emap_out [m] (may be NULL): old engine index -> new.
int mcf_topology_merge_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, int64_t k, const int32_t* ntail,
                            const int32_t* nhead, int32_t* orig_out, int32_t* tail_out, int32_t* head_out, int64_t* bucket_off_out,
                            int64_t* adj_off_out, int64_t* adj_out, int32_t* emap_out) {
    if (k < 0) return -1;
    McfHostImage im;
    const int rc = build(n, m, tail, head, im);
    if (rc) return rc;
    for (int64_t i = 0; i < k; ++i) if (ntail[i] < 0 || ntail[i] >= n || nhead[i] < 0 || nhead[i] >= n || ntail[i] == nhead[i]) return -1;
    const int64_t per = mcf_topo_per(n);
    std::vector<int64_t> perm((size_t)k);
    for (int64_t i = 0; i < k; ++i) perm[(size_t)i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return mcf_topo_key(ntail[a], nhead[a], per) < mcf_topo_key(ntail[b], nhead[b], per); });
    std::vector<int64_t> nkey((size_t)k), npos((size_t)k);
    for (int64_t r = 0; r < k; ++r) nkey[(size_t)r] = mcf_topo_key(ntail[perm[(size_t)r]], nhead[perm[(size_t)r]], per);
    std::vector<int32_t> emap((size_t)m);
    // arcs: last to first, so that no loop order is relied upon
    for (int64_t e = m; e-- > 0;) {
        const int64_t d = mcf_topo_old_index(e, mcf_topo_key(im.tail[(size_t)e], im.head[(size_t)e], per), nkey.data(), k);
        emap[(size_t)e] = (int32_t)d;
        orig_out[d] = im.orig[(size_t)e]; tail_out[d] = im.tail[(size_t)e]; head_out[d] = im.head[(size_t)e];
    }
    for (int64_t r = k; r-- > 0;) {
        const int64_t d = mcf_topo_new_index(r, nkey[(size_t)r], im.tail.data(), im.bucket_off);
        npos[(size_t)r] = d;
        orig_out[d] = (int32_t)(m + perm[(size_t)r]); tail_out[d] = ntail[perm[(size_t)r]]; head_out[d] = nhead[perm[(size_t)r]];
    }
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) bucket_off_out[x] = im.bucket_off[x] + mcf_count_below(nkey.data(), k, (int64_t)x << 32);
    // adjacency: the 2k end points sorted by node
    const int64_t k2 = 2 * k;
    std::vector<int64_t> ep((size_t)k2), ep_node((size_t)k2), ep_end((size_t)k2);
    for (int64_t r = 0; r < k; ++r) {
        const int64_t i = perm[(size_t)r];
        ep[(size_t)(2 * r)] = ((int64_t)ntail[i] << 32) | (r << 1) | 1;
        ep[(size_t)(2 * r + 1)] = ((int64_t)nhead[i] << 32) | (r << 1);
    }
    std::sort(ep.begin(), ep.end());
    for (int64_t j = 0; j < k2; ++j) { ep_node[(size_t)j] = ep[(size_t)j] >> 32; ep_end[(size_t)j] = im.adj_off[(size_t)(ep[(size_t)j] >> 32) + 1]; }
    for (int32_t u = 0; u <= n; ++u) adj_off_out[u] = mcf_topo_adj_off(im.adj_off[(size_t)u], u, ep_node.data(), k2);
    for (int64_t p = 2 * m; p-- > 0;) {
        const int64_t x = im.adj[(size_t)p];
        const int64_t e = (x & 0xffffffffll) >> 1;
        adj_out[mcf_topo_adj_index(p, ep_end.data(), k2)] = (x & ~0xfffffffell) | ((int64_t)emap[(size_t)e] << 1);
    }
    for (int64_t j = 0; j < k2; ++j) {
        const int64_t r = (ep[(size_t)j] & 0xffffffffll) >> 1, is_tail = ep[(size_t)j] & 1, i = perm[(size_t)r];
        adj_out[ep_end[(size_t)j] + j] = ((int64_t)(is_tail ? nhead[i] : ntail[i]) << 32) | (npos[(size_t)r] << 1) | is_tail;
    }
    if (emap_out) for (int64_t e = 0; e < m; ++e) emap_out[e] = emap[(size_t)e];
    return 0;
}

}  // extern "C"
