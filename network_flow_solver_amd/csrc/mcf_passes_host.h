// mcf_passes_host.h -- host drivers of the post-solve passes on a resident handle (kernels: mcf_passes_dev.h).  Not a header
// of its own: mcf_engine.hip includes it after the handle and its launch helpers.

namespace {

// ---- scratch the passes allocate on first use
// One member of a group: where the pointer lives and how much it holds.
struct LazyBuf {
    void** p;
    size_t bytes;
    template <typename T>
    LazyBuf(T** q, size_t count) : p(reinterpret_cast<void**>(q)), bytes((count ? count : 1) * sizeof(T)) {}
};
void lazy_release(std::initializer_list<LazyBuf> g) {
    for (const LazyBuf& b : g) { (void)hipFree(*b.p); *b.p = nullptr; }
}
// all members (`scale` times their size) or none: every member null again and the sticky HIP error cleared when one cannot be had
int lazy_alloc(mcf_handle* h, const char* what, std::initializer_list<LazyBuf> g, size_t scale) {
    for (const LazyBuf& b : g) {
        if (hipMalloc(b.p, b.bytes * scale) == hipSuccess) continue;
        (void)hipGetLastError();
        lazy_release(g);
        h->err = std::string("hipMalloc ") + what;
        return MCF_E_ALLOC;
    }
    return MCF_OK;
}
// A group is complete or absent, so its first pointer says which.
int lazy_group(mcf_handle* h, const char* what, std::initializer_list<LazyBuf> g) {
    return *g.begin()->p ? MCF_OK : lazy_alloc(h, what, g, 1);
}
// Arrays of *cap entries (a member's count: its elements per entry), replaced by half as large again when `want` do not fit.
int lazy_grow(mcf_handle* h, const char* what, int64_t* cap, int64_t want, std::initializer_list<LazyBuf> g) {
    if (want <= *cap) return MCF_OK;
    lazy_release(g);
    *cap = 0;
    const int64_t grown = want + want / 2 + 1024;
    const int rc = lazy_alloc(h, what, g, (size_t)grown);
    if (rc == MCF_OK) *cap = grown;
    return rc;
}

// the full node -> arc adjacency: the handle's own where it holds one for all arcs, else the certificate's (cert_prepare)
struct FullAdj { bool own; const int64_t *off, *adj; };
FullAdj full_adj(const mcf_handle* h) {
    const bool own = h->d_adj && !h->view.rc_partial;   // (h->view.adj goes away with dropped reduced costs; the arrays stay)
    return {own, own ? h->d_adj_off : h->d_ct_adj_off, own ? h->d_adj : h->d_ct_adj};
}

// workgroups of a one-lane-per-item pass over `count` nodes (grid-stride beyond kCertMaxBlocks)
int node_grid(int64_t count) {
    const int64_t nb = (count + kCertThreads - 1) / kCertThreads;
    return (int)(nb < kCertMaxBlocks ? nb : kCertMaxBlocks);
}

// ---- certificate on the device: host helpers
void put128(int64_t* hi_lo, __int128 x) { hi_lo[0] = (int64_t)(x >> 64); hi_lo[1] = (int64_t)(uint64_t)x; }

// the caller's flows (caller's order, as they are) into the scratch buffer; nullptr stays nullptr
int cert_upload_flow(mcf_handle* h, const int64_t* flow, const int64_t** dev) {
    *dev = nullptr;
    if (!flow || h->im.m == 0) return MCF_OK;
    const int rc = lazy_group(h, "certificate flows", {{&h->d_ct_flow, (size_t)h->im.m}});
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_ct_flow, flow, (size_t)h->im.m * 8, hipMemcpyHostToDevice, h->stream));
    *dev = h->d_ct_flow;
    return MCF_OK;
}

// what the certificate needs beyond the solver's arrays: supplies, a FULL adjacency (need_adj), partial buffers, events
int cert_prepare(mcf_handle* h, bool need_adj = true) {
    const McfHostImage& im = h->im;
    int rc;
    if (!h->d_ct_supply) {
        if ((rc = lazy_group(h, "supplies", {{&h->d_ct_supply, (size_t)im.n}})) != MCF_OK) return rc;
        if (hipMemcpy(h->d_ct_supply, im.supply.data(), (size_t)im.n * 8, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError(); lazy_release({{&h->d_ct_supply, 0}}); h->err = "hipMemcpy supplies"; return MCF_E_HIP;
        }
    }
    if (need_adj && !full_adj(h).own && !h->d_ct_adj_off) {
        std::vector<int64_t> off((size_t)im.n + 1, 0), adj((size_t)(2 * im.m));
        for (int64_t e = 0; e < im.m; ++e) { off[(size_t)im.tail[e] + 1]++; off[(size_t)im.head[e] + 1]++; }
        for (int32_t u = 0; u < im.n; ++u) off[(size_t)u + 1] += off[u];
        std::vector<int64_t> fill(off.begin(), off.end() - 1);
        for (int64_t e = 0; e < im.m; ++e) {
            const int64_t t = im.tail[e], hd = im.head[e];
            adj[(size_t)fill[t]++] = (hd << 32) | (e << 1) | 1;
            adj[(size_t)fill[hd]++] = (t << 32) | (e << 1);
        }
        if ((rc = lazy_group(h, "certificate adjacency", {{&h->d_ct_adj_off, off.size()}, {&h->d_ct_adj, adj.size()}})) != MCF_OK) return rc;
        if (hipMemcpy(h->d_ct_adj_off, off.data(), off.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
            (!adj.empty() && hipMemcpy(h->d_ct_adj, adj.data(), adj.size() * 8, hipMemcpyHostToDevice) != hipSuccess)) {
            (void)hipGetLastError(); lazy_release({{&h->d_ct_adj_off, 0}, {&h->d_ct_adj, 0}});
            h->err = "hipMemcpy certificate adjacency"; return MCF_E_HIP;
        }
    }
    if ((rc = lazy_group(h, "certificate partials", {{&h->d_ct_arc, kCertMaxBlocks + 1}, {&h->d_ct_node, kCertMaxBlocks + 1},
                                                      {&h->d_ct_csum, (size_t)im.n_nodes}})) != MCF_OK) return rc;
    for (hipEvent_t& e : h->ct_ev) if (!e) HIP_TRY(h, hipEventCreate(&e));
    return MCF_OK;
}

// ---- shared by mcf_update_costs and mcf_update_rhs
unsigned uc_blocks_for(int64_t items) { const int64_t b = (items + kUcThreads - 1) / kUcThreads; return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); }

// caller's arc index -> engine arc index, and the stamps that resolve duplicates (arcs and nodes)
void uc_index(mcf_handle* h) {
    const McfHostImage& im = h->im;
    if (!h->uc_inv.empty() || im.m == 0) return;
    h->uc_inv.assign((size_t)im.m, 0);
    for (int64_t e = 0; e < im.m; ++e) h->uc_inv[(size_t)im.orig[(size_t)e]] = (int32_t)e;
    h->uc_stamp.assign((size_t)im.m, 0);
}
void uc_next_gen(mcf_handle* h) {
    if (h->rhs_nstamp.empty()) h->rhs_nstamp.assign((size_t)h->im.n, 0);
    if (++h->uc_gen == 0) {
        std::fill(h->uc_stamp.begin(), h->uc_stamp.end(), 0u);
        std::fill(h->rhs_nstamp.begin(), h->rhs_nstamp.end(), 0u);
        h->uc_gen = 1;
    }
}

// jump records (double buffered) and the info words
int uc_alloc(mcf_handle* h) {
    const size_t N = (size_t)h->im.n_nodes;
    return lazy_group(h, "jump records", {{&h->d_uc_jump[0], N}, {&h->d_uc_jump[1], N}, {&h->d_uc_info, 2}});
}

// potentials from the seeded records in d_uc_jump[0]: rounds = ceil(log2(greatest depth)), at least the final one
void uc_jump_rounds(mcf_handle* h, int32_t depth) {
    const int32_t N = h->im.n_nodes;
    hipStream_t s = h->stream;
    int rounds = 1;
    while (((int64_t)1 << rounds) < (int64_t)depth) ++rounds;
    int cur = 0;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(r + 1 < rounds ? k_uc_jump<false> : k_uc_jump<true>, dim3(uc_blocks_for(N)), dim3(kUcThreads), 0, s, (const McfJump*)h->d_uc_jump[cur], h->d_uc_jump[cur ^ 1], h->d_pi, N);
        cur ^= 1;
    }
}

// The tail of both calls: resident reduced costs / key codes from the potentials (`rebuild`; only where the handle keeps
// them), everything derived for pricing starts over, the control block says "running" again with its counters kept.
// *h_ctx must be current (sync_ctx, and nothing since has touched the device's copy).
int uc_finish(mcf_handle* h, bool rebuild) {
    const McfHostImage& im = h->im;
    hipStream_t s = h->stream;
    if (rebuild && h->rcached) {   // (a handle that dropped its reduced costs, or never kept any, prices from the potentials)
        int64_t pb = (im.m_pad / 4 / MCF_NUM_BUCKETS + kUcThreads * kUcUnroll - 1) / (kUcThreads * kUcUnroll);
        pb = pb < 1 ? 1 : (pb > 2048 / MCF_NUM_BUCKETS ? 2048 / MCF_NUM_BUCKETS : pb);
        hipLaunchKernelGGL(k_uc_rebuild, dim3((unsigned)pb * MCF_NUM_BUCKETS), dim3(kUcThreads), 0, s, h->view, im.m_pad);
    }
    // derived pricing state: candidate list and cache, clean / dirty marks, Devex weights, block cursor, tuner
    HIP_TRY(h, hipMemsetAsync(h->d_cand, 0xff, kMaxPriceBlocks * sizeof(McfCand), s));
    if (h->d_candx) HIP_TRY(h, hipMemsetAsync(h->d_candx, 0xff, kMaxPriceBlocks * sizeof(McfCandX), s));
    if (h->d_dirty) HIP_TRY(h, hipMemsetAsync(h->d_dirty->flag, 1, sizeof(h->d_dirty->flag), s));
    if (h->opt.rule == MCF_RULE_DEVEX_BLOCK) hipLaunchKernelGGL(k_uc_ones, dim3(uc_blocks_for(im.m_pad / 4)), dim3(kUcThreads), 0, s, reinterpret_cast<float4*>(h->d_weight), im.m_pad / 4);
    HIP_TRY(h, hipGetLastError());
    {
        McfCtx& c = *h->h_ctx;
        c.status = MCF_RUNNING;
        c.limit_checked = 0;
        c.unbounded_arc = -1;
        c.minor_left = 0;
        mcf_init_block_state(&c, h->opt.rule, im.m, h->opt.block_size);
        if (h->opt.rule == MCF_RULE_DEVEX_BLOCK) {
            if (h->opt.devex_tuner > 0) c.auto_tune = 1; else if (h->opt.devex_tuner < 0) c.auto_tune = 0;
            if (h->opt.devex_stay > 0) c.devex_cyclic = 0;
        }
        HIP_TRY(h, hipMemcpyAsync(h->d_ctx, h->h_ctx, sizeof(McfCtx), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    h->ctx_current = false;
    return MCF_OK;
}

}  // namespace

extern "C" {

// Re-optimise after a cost change: the resident basis stays, potentials / reduced costs / key codes follow the new costs
// (kernels k_uc_* above).  Everything is validated on the host before the first byte moves.
int mcf_update_costs(mcf_handle* h, int64_t count, const int64_t* arc, const int64_t* new_cost) {
    if (!h) return MCF_E_BAD_ARG;
    if (h->shards != 1) {
        h->err = "mcf_update_costs: handle was created with shard_count > 1; sharded handles cannot change their costs";
        return MCF_E_STATE;
    }
    if (count < 0 || (count > 0 && (!arc || !new_cost))) { h->err = "mcf_update_costs: bad count / null array"; return MCF_E_BAD_ARG; }
    McfHostImage& im = h->im;
    for (int64_t i = 0; i < count; ++i)
        if (arc[i] < 0 || arc[i] >= im.m) { h->err = "mcf_update_costs: arc index out of range"; return MCF_E_BAD_ARG; }
    for (int64_t i = 0; i < count; ++i)
        if (new_cost[i] > INT32_MAX || new_cost[i] < -(int64_t)INT32_MAX) { h->err = "mcf_update_costs: |cost| must fit int32"; return MCF_E_RANGE; }
    uc_index(h);
    uc_next_gen(h);
    // duplicates: the last entry wins (walk backwards, keep the first sighting of every arc)
    std::vector<int32_t> ue, uc;
    ue.reserve((size_t)count); uc.reserve((size_t)count);
    int64_t max_abs = 0;
    for (int64_t i = count - 1; i >= 0; --i) {
        const int32_t e = h->uc_inv[(size_t)arc[i]];
        if (h->uc_stamp[(size_t)e] == h->uc_gen) continue;
        h->uc_stamp[(size_t)e] = h->uc_gen;
        ue.push_back(e); uc.push_back((int32_t)new_cost[i]);
        const int64_t a = new_cost[i] < 0 ? -new_cost[i] : new_cost[i];
        if (a > max_abs) max_abs = a;
    }
    // big-M never shrinks; it grows when a new cost needs it (same rule as mcf_build_image)
    int64_t big_m = im.big_m;
    if ((max_abs + 1) * ((int64_t)im.n + 2) > big_m) big_m = (max_abs + 1) * ((int64_t)im.n + 2);
    if (big_m >= ((int64_t)1 << 44)) { h->err = "mcf_update_costs: max|cost| * n too large for big-M"; return MCF_E_RANGE; }
    const int64_t d_bigm = big_m - im.big_m;
    const int64_t nu = (int64_t)ue.size();

    HIP_TRY(h, hipSetDevice(h->device));
    int rc = uc_alloc(h);   // temporaries
    if (rc) return rc;
    if ((rc = lazy_grow(h, "cost changes", &h->uc_cap, nu, {{&h->d_uc_arc, 1}, {&h->d_uc_cost, 1}})) != MCF_OK) return rc;
    rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    if (h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "mcf_update_costs: the handle's tree is not usable"; return MCF_E_STATE; }

    hipStream_t s = h->stream;
    const int32_t N = im.n_nodes;
    if (nu > 0) {
        HIP_TRY(h, hipMemcpyAsync(h->d_uc_arc, ue.data(), (size_t)nu * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->d_uc_cost, uc.data(), (size_t)nu * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipMemsetAsync(h->d_uc_info, 0, 2 * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_uc_seed, dim3(uc_blocks_for(N)), dim3(kUcThreads), 0, s, (const McfNode*)h->d_node, N, im.m, d_bigm, h->d_uc_jump[0], h->d_uc_info);
    if (nu > 0)
        hipLaunchKernelGGL(k_uc_scatter, dim3(uc_blocks_for(nu)), dim3(kUcThreads), 0, s, nu, (const int32_t*)h->d_uc_arc, (const int32_t*)h->d_uc_cost,
                           h->d_cost, (const int8_t*)h->d_state, (const int32_t*)h->d_tail, (const int32_t*)h->d_head, (const McfNode*)h->d_node,
                           h->d_uc_jump[0], h->d_uc_info);
    HIP_TRY(h, hipGetLastError());
    int32_t info[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(info, h->d_uc_info, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));   // (also: the pageable sources above are free again)
    // potentials: only when a tree arc changed (or big-M grew)
    if (info[1] > 0 || d_bigm != 0) uc_jump_rounds(h, info[0]);
    // the view's big-M first: the key codes below are formed with it, and captured graphs carry the view by value
    if (d_bigm != 0) {
        h->view.vk_bigm = big_m;
        drop_graph(h);
    }
    rc = uc_finish(h, true);
    if (rc) return rc;
    // host image: a later mcf_reset / mcf_set_basis (which rebuild its potentials and reduced costs from these) and the
    // objective of mcf_get_result use the new costs
    for (int64_t i = 0; i < nu; ++i) { im.cost[(size_t)ue[(size_t)i]] = uc[(size_t)i]; im.cost64[(size_t)ue[(size_t)i]] = uc[(size_t)i]; }
    im.big_m = big_m;
    return MCF_OK;
}

// Re-optimise after supplies / capacities changed (kernels k_rhs_* above).  Non-basic flows follow their capacities, tree
// flows are recomputed as subtree sums of the node balances, and a census decides: the basis stays (path 0), is repaired
// on the host at mcf_set_basis cost (path 1, mcf_repair_basis), or the handle goes to the cold start (path 2).
int mcf_update_rhs(mcf_handle* h, int64_t n_sup, const int64_t* node, const int64_t* new_supply, int64_t n_cap,
                   const int64_t* arc, const int64_t* new_cap, mcf_rhs_report* out) {
    if (!h) return MCF_E_BAD_ARG;
    if (h->shards != 1) {
        h->err = "mcf_update_rhs: handle was created with shard_count > 1; sharded handles cannot change their supplies / capacities";
        return MCF_E_STATE;
    }
    if (n_sup < 0 || n_cap < 0 || (n_sup > 0 && (!node || !new_supply)) || (n_cap > 0 && (!arc || !new_cap))) {
        h->err = "mcf_update_rhs: bad count / null array";
        return MCF_E_BAD_ARG;
    }
    McfHostImage& im = h->im;
    for (int64_t i = 0; i < n_sup; ++i)
        if (node[i] < 0 || node[i] >= im.n) { h->err = "mcf_update_rhs: node index out of range"; return MCF_E_BAD_ARG; }
    for (int64_t i = 0; i < n_cap; ++i)
        if (arc[i] < 0 || arc[i] >= im.m) { h->err = "mcf_update_rhs: arc index out of range"; return MCF_E_BAD_ARG; }
    uc_index(h);
    uc_next_gen(h);
    // duplicates: the last entry wins (walk backwards, keep the first sighting); nodes first, then arcs, in one pair of arrays
    std::vector<int32_t> idx;
    std::vector<int64_t> val;
    idx.reserve((size_t)(n_sup + n_cap)); val.reserve((size_t)(n_sup + n_cap));
    __int128 total = 0, positive = 0;
    for (int32_t v = 0; v < im.n; ++v) if (im.supply[(size_t)v] > 0) positive += im.supply[(size_t)v];
    for (int64_t i = n_sup - 1; i >= 0; --i) {
        const int32_t v = (int32_t)node[i];
        if (h->rhs_nstamp[(size_t)v] == h->uc_gen) continue;
        h->rhs_nstamp[(size_t)v] = h->uc_gen;
        idx.push_back(v); val.push_back(new_supply[i]);
        const int64_t was = im.supply[(size_t)v];
        total += (__int128)new_supply[i] - was;
        positive += (__int128)(new_supply[i] > 0 ? new_supply[i] : 0) - (was > 0 ? was : 0);
    }
    if (total != 0) { h->err = "mcf_update_rhs: supplies do not balance"; return MCF_E_RANGE; }
    if (positive >= (__int128)MCF_INF) { h->err = "mcf_update_rhs: the sum of the positive supplies must stay below 2^60"; return MCF_E_RANGE; }
    const int64_t ns = (int64_t)idx.size();
    for (int64_t i = n_cap - 1; i >= 0; --i) {
        const int32_t e = h->uc_inv[(size_t)arc[i]];
        if (h->uc_stamp[(size_t)e] == h->uc_gen) continue;
        h->uc_stamp[(size_t)e] = h->uc_gen;
        idx.push_back(e); val.push_back((new_cap[i] < 0 || new_cap[i] >= MCF_INF) ? MCF_INF : new_cap[i]);
    }
    const int64_t nc = (int64_t)idx.size() - ns;

    HIP_TRY(h, hipSetDevice(h->device));
    int rc = uc_alloc(h);
    if (rc) return rc;
    if ((rc = cert_prepare(h)) != MCF_OK) return rc;   // device supplies, a full adjacency, two events
    const int32_t N = im.n_nodes;
    const int64_t chunks = ((int64_t)N + kRhsChunk - 1) / kRhsChunk;
    if ((rc = lazy_group(h, "balances", {{&h->d_rhs_bal, (size_t)N}, {&h->d_rhs_part, (size_t)chunks}, {&h->d_rhs_info, (size_t)RHS_COUNTERS}})) != MCF_OK) return rc;
    if ((rc = lazy_grow(h, "supply / capacity changes", &h->rhs_cap, ns + nc, {{&h->d_rhs_idx, 1}, {&h->d_rhs_val, 1}})) != MCF_OK) return rc;
    rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    if (h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "mcf_update_rhs: the handle's tree is not usable"; return MCF_E_STATE; }

    // ---- device passes
    hipStream_t s = h->stream;
    const int32_t cur = tree_sel(*h->h_ctx).cur;
    const FullAdj fa = full_adj(h);
    McfView vw = h->view;
    if (h->rcached) { vw.rcache = h->d_rcache; } else { vw.vkey = nullptr; }   // (key codes are patched only where they are kept)
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
    if (ns + nc > 0) {
        HIP_TRY(h, hipMemcpyAsync(h->d_rhs_idx, idx.data(), (size_t)(ns + nc) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->d_rhs_val, val.data(), (size_t)(ns + nc) * 8, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipMemsetAsync(h->d_rhs_info, 0, RHS_COUNTERS * sizeof(unsigned long long), s));
    HIP_TRY(h, hipMemsetAsync(h->d_uc_info, 0, 2 * sizeof(int32_t), s));
    HIP_TRY(h, hipMemsetAsync(h->d_rhs_bal, 0, (size_t)N * sizeof(mcf_u128), s));
    if (ns + nc > 0)
        hipLaunchKernelGGL(k_rhs_scatter, dim3(uc_blocks_for(ns > nc ? ns : nc)), dim3(kRhsThreads), 0, s, vw, ns, (const int32_t*)h->d_rhs_idx,
                           (const int64_t*)h->d_rhs_val, h->d_ct_supply, nc, (const int32_t*)(h->d_rhs_idx + ns), (const int64_t*)(h->d_rhs_val + ns), h->d_rhs_info);
    hipLaunchKernelGGL(k_rhs_balance, dim3(uc_blocks_for(N)), dim3(kRhsThreads), 0, s, vw, cur, (const int64_t*)h->d_ct_supply,
                       fa.off, fa.adj, h->d_rhs_bal);
    hipLaunchKernelGGL(k_rhs_scan_totals, dim3((unsigned)chunks), dim3(kRhsThreads), 0, s, (const mcf_u128*)h->d_rhs_bal, N, h->d_rhs_part);
    hipLaunchKernelGGL((k_scan_chunks<mcf_u128, mcf_u128>), dim3(1), dim3(1024), 0, s, (const mcf_u128*)h->d_rhs_part, chunks, h->d_rhs_part, (mcf_u128*)nullptr);
    hipLaunchKernelGGL(k_rhs_scan_apply, dim3((unsigned)chunks), dim3(kRhsThreads), 0, s, h->d_rhs_bal, N, (const mcf_u128*)h->d_rhs_part);
    // jump records for the potentials below an artificial arc that turns round (seeded with 0; the flow pass marks the turns)
    hipLaunchKernelGGL(k_uc_seed, dim3(uc_blocks_for(N)), dim3(kUcThreads), 0, s, (const McfNode*)h->d_node, N, im.m, (int64_t)0, h->d_uc_jump[0], h->d_uc_info);
    hipLaunchKernelGGL(k_rhs_flows, dim3(uc_blocks_for(N)), dim3(kRhsThreads), 0, s, vw, cur, (const mcf_u128*)h->d_rhs_bal, im.big_m, h->d_uc_jump[0], h->d_rhs_info);
    HIP_TRY(h, hipGetLastError());
    unsigned long long info[RHS_COUNTERS] = {0, 0, 0, 0};
    int32_t depth[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(info, h->d_rhs_info, sizeof info, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(depth, h->d_uc_info, sizeof depth, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));   // (also: the pageable sources above are free again)

    // host image: the objective, a later mcf_reset / mcf_set_basis and the repair below use the new data
    for (int64_t i = 0; i < ns; ++i) im.supply[(size_t)idx[(size_t)i]] = val[(size_t)i];
    for (int64_t i = ns; i < ns + nc; ++i) im.arcw[(size_t)idx[(size_t)i]].cap = val[(size_t)i];

    mcf_rhs_report rep;
    std::memset(&rep, 0, sizeof rep);
    rep.tree_violations = (int64_t)info[RHS_VIOL];
    rep.wrong_way = (int64_t)info[RHS_WRONG];
    rep.art_flips = (int64_t)info[RHS_FLIPS];
    rep.upper_moved = (int64_t)info[RHS_MOVED];
    if (rep.tree_violations == 0 && rep.wrong_way == 0) {
        // ---- path 0: the basis stays
        if (rep.art_flips > 0) uc_jump_rounds(h, depth[0]);
        if ((rc = uc_finish(h, rep.art_flips > 0)) != MCF_OK) return rc;
        HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
        HIP_TRY(h, hipEventSynchronize(h->ct_ev[1]));
    } else {
        // ---- path 1: states and node records come down, the basis is repaired on the host and installed as mcf_set_basis
        // does; path 2 (cold start) when the repair refuses
        HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
        std::vector<int8_t> st((size_t)im.m_pad), in_tree((size_t)(im.m ? im.m : 1), 0), at_upper((size_t)(im.m ? im.m : 1), 0), hang((size_t)im.n, 0);
        std::vector<McfNode> nodes((size_t)N);
        HIP_TRY(h, hipMemcpy(st.data(), h->d_state, st.size(), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(nodes.data(), h->d_node, nodes.size() * sizeof(McfNode), hipMemcpyDeviceToHost));
        for (int64_t e = 0; e < im.m; ++e) {
            in_tree[(size_t)im.orig[(size_t)e]] = st[(size_t)e] == 0;
            at_upper[(size_t)im.orig[(size_t)e]] = st[(size_t)e] == -1;
        }
        for (int32_t v = 0; v < im.n; ++v) hang[(size_t)v] = nodes[(size_t)v].pred >= 0 && (int64_t)(nodes[(size_t)v].pred >> 1) >= im.m;
        McfRepairReport rr;
        const std::string msg = mcf_repair_basis(im, in_tree.data(), at_upper.data(), hang.data(), &rr);
        rep.path = 1;
        rep.arcs_cut = rr.arcs_cut;
        rep.repair_rounds = rr.rounds;
        if (!msg.empty()) { mcf_init_cold_basis(im); rep.path = 2; rep.arcs_cut = 0; }
        mcf_refresh_rcache(im);
        // the counters keep counting: upload_image starts them over, so they are carried across it
        const McfCtx was = *h->h_ctx;
        const mcf_stats stats_was = h->stats;
        if ((rc = upload_image(h)) != MCF_OK) return rc;
        McfCtx& c = *h->h_ctx;
        c.pivots = was.pivots; c.degenerate = was.degenerate; c.bound_flips = was.bound_flips; c.arcs_priced = was.arcs_priced;
        c.nodes_moved = was.nodes_moved; c.subtree_nodes = was.subtree_nodes; c.cycle_arcs = was.cycle_arcs;
        c.scans = was.scans; c.scan_rounds = was.scan_rounds; c.minor_pivots = was.minor_pivots; c.major_sweeps = was.major_sweeps;
        c.rebuilds = was.rebuilds;
        const int64_t price_bytes = h->stats.price_bytes;
        h->stats = stats_was;
        h->stats.price_bytes = price_bytes;
        h->stats.rc_dropped_at = 0; h->stats.run_left_at = 0;   // (a fresh image keeps its reduced costs and its run shape again)
        h->sw_pivots = c.pivots; h->sw_subtree = c.subtree_nodes; h->run_seen = c.pivots;
        HIP_TRY(h, hipMemsetAsync(h->d_cand, 0xff, kMaxPriceBlocks * sizeof(McfCand), s));
        if (h->d_candx) HIP_TRY(h, hipMemsetAsync(h->d_candx, 0xff, kMaxPriceBlocks * sizeof(McfCandX), s));
        HIP_TRY(h, hipMemcpyAsync(h->d_ctx, h->h_ctx, sizeof(McfCtx), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        h->ctx_current = true;
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ct_ev[0], h->ct_ev[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
    rep.device_ms = ms;
    if (out) *out = rep;
    return MCF_OK;
}

// ---- certificate on the device (include/mcf.h)
int mcf_certify(mcf_handle* h, const int64_t* flow, const int64_t* potential, uint32_t checks, mcf_certificate* out) {
    if (!h || !out || (checks & ~MCF_CERT_ALL)) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    const McfHostImage& im = h->im;
    if (!checks) checks = MCF_CERT_ALL;
    if (flow || potential) checks &= ~(MCF_CERT_BASIS | MCF_CERT_PRICING);
    std::vector<int64_t> pi_host;   // (outlives the asynchronous copy: the call ends with a synchronisation)
    if (potential) {
        pi_host.assign((size_t)im.n_nodes, 0);
        for (int32_t v = 0; v < im.n; ++v) {
            if (potential[v] > ((int64_t)1 << 61) || potential[v] < -((int64_t)1 << 61)) { h->err = "mcf_certify: |potential| must not exceed 2^61"; return MCF_E_RANGE; }
            pi_host[(size_t)v] = potential[v];
        }
    }
    if ((rc = cert_prepare(h)) != MCF_OK) return rc;
    CertArgs a;
    std::memset(&a, 0, sizeof a);
    if ((rc = cert_upload_flow(h, flow, &a.cflow)) != MCF_OK) return rc;
    a.pi = h->d_pi;
    if (potential) {
        if ((rc = lazy_group(h, "certificate potentials", {{&h->d_ct_pi, (size_t)im.n_nodes}})) != MCF_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_ct_pi, pi_host.data(), pi_host.size() * 8, hipMemcpyHostToDevice, h->stream));
        a.pi = h->d_ct_pi;
    }
    a.supply = h->d_ct_supply;
    a.adj_off = full_adj(h).off;
    a.adj = full_adj(h).adj;
    a.rcache = (checks & MCF_CERT_PRICING) && h->rcached ? h->d_rcache : nullptr;
    a.vkey = (checks & MCF_CERT_PRICING) && h->rcached ? h->view.vkey : nullptr;
    a.csum = h->d_ct_csum;
    a.checks = checks;
    a.resident_flow = flow ? 0 : 1;
    a.cur = tree_sel(*h->h_ctx).cur;
    a.arena = tree_sel(*h->h_ctx).arena;
    a.partial = h->view.rc_partial;
    a.shard = h->shard; a.shards = h->shards;
    a.bigm = im.big_m;
    const int ab = mcf_price_blocks(im.m, 1, 0);
    const int nb = node_grid(im.n_nodes);
    hipStream_t s = h->stream;
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
    hipLaunchKernelGGL(im.m >= kIncrementalMinArcs ? k_cert_arcs<true> : k_cert_arcs<false>, dim3(ab), dim3(kCertThreads), 0, s, h->view, a, h->d_ct_arc);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    if (checks & MCF_CERT_BASIS) {
        HIP_TRY(h, hipMemsetAsync(h->d_ct_csum, 0, (size_t)im.n_nodes * 4, s));
        hipLaunchKernelGGL(k_cert_child, dim3(nb), dim3(kCertThreads), 0, s, h->view, h->d_ct_csum);
    }
    hipLaunchKernelGGL(k_cert_nodes, dim3(nb), dim3(kCertThreads), 0, s, h->view, a, h->d_ct_node);
    HIP_TRY(h, hipEventRecord(h->ct_ev[2], s));
    hipLaunchKernelGGL(k_cert_final, dim3(1), dim3(kCertThreads), 0, s, h->d_ct_arc, ab, h->d_ct_node, nb);
    HIP_TRY(h, hipGetLastError());
    McfCertArcAcc A;
    McfCertNodeAcc N;
    HIP_TRY(h, hipMemcpyAsync(&A, h->d_ct_arc + ab, sizeof A, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(&N, h->d_ct_node + nb, sizeof N, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    float ms_a = 0, ms_n = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms_a, h->ct_ev[0], h->ct_ev[1]));
    HIP_TRY(h, hipEventElapsedTime(&ms_n, h->ct_ev[1], h->ct_ev[2]));

    mcf_certificate c;
    std::memset(&c, 0, sizeof c);
    auto idx = [](int64_t i) { return i == MCF_CERT_NONE ? (int64_t)-1 : i; };
    c.checks = checks;
    c.negative_flow_count = A.neg_n; c.over_capacity_count = A.over_n; c.bounds_worst = A.bnd_w; c.bounds_worst_arc = idx(A.bnd_i);
    c.imbalance_count = N.imb_n; c.imbalance_worst = N.imb_w; c.imbalance_worst_node = idx(N.imb_i);
    c.dual_lower_count = A.dlo_n; c.dual_lower_worst = A.dlo_w; c.dual_lower_arc = idx(A.dlo_i);
    c.dual_upper_count = A.dup_n; c.dual_upper_worst = A.dup_w; c.dual_upper_arc = idx(A.dup_i);
    const int64_t art_resident = (int64_t)N.art_lo;   // (below 2^60: "Numeric domain")
    c.artificial_flow = flow ? 0 : art_resident;
    c.big_m = im.big_m;
    const __int128 primal = (__int128)(((mcf_u128)A.primal_hi << 64) | A.primal_lo);
    const __int128 bigm_term = (__int128)c.big_m * c.artificial_flow;
    const __int128 dual = (__int128)((((mcf_u128)N.dnode_hi << 64) | N.dnode_lo) + (((mcf_u128)A.dcap_hi << 64) | A.dcap_lo));
    const __int128 gap = primal + bigm_term - dual;
    if (checks & MCF_CERT_OBJECTIVES) { put128(c.primal, primal); put128(c.bigm_term, bigm_term); put128(c.dual, dual); put128(c.gap, gap); }
    c.basic_arcs = A.basic_n + N.art_basic;
    c.basic_count_mismatch = (checks & MCF_CERT_BASIS) && c.basic_arcs != im.n ? 1 : 0;
    c.tree_rc_count = N.tree_rc_bad; c.state_flow_count = A.stf_n; c.tree_shape_count = N.shape_bad; c.strong_count = N.strong_bad;
    c.rc_compared = A.rc_n; c.rc_mismatch_count = A.rc_bad; c.key_compared = A.key_n; c.key_mismatch_count = A.key_bad;
    c.saturated_arcs = A.sat_n;
    c.arc_pass_ms = ms_a; c.node_pass_ms = ms_n;
    const int32_t st = h->h_ctx->status;
    c.status = st == MCF_RUNNING ? -1 : st == MCF_UNBOUNDED ? MCF_ST_UNBOUNDED
               : st == MCF_OPTIMAL ? (art_resident > 0 ? MCF_ST_INFEASIBLE : MCF_ST_OPTIMAL) : MCF_ST_ITERATION_LIMIT;
    const uint32_t need = MCF_CERT_BOUNDS | MCF_CERT_CONSERVATION | MCF_CERT_DUAL | MCF_CERT_OBJECTIVES;
    c.verdict = MCF_CERT_NOT_PROVEN;
    if ((checks & need) == need && !A.neg_n && !A.over_n && !N.imb_n && !A.dlo_n && !A.dup_n && gap == 0)
        c.verdict = c.artificial_flow > 0 ? MCF_CERT_INFEASIBLE : MCF_CERT_OPTIMAL;
    c.proves_status = (c.status == MCF_ST_OPTIMAL && c.verdict == MCF_CERT_OPTIMAL) || (c.status == MCF_ST_INFEASIBLE && c.verdict == MCF_CERT_INFEASIBLE) ? 1 : 0;
    *out = c;
    return MCF_OK;
}

int mcf_bottlenecks(mcf_handle* h, const int64_t* flow, int64_t num, int64_t den, int64_t* idx_out, int64_t idx_cap, int64_t* count) {
    if (!h || !count || num < 0 || den <= 0 || idx_cap < 0 || (idx_cap > 0 && !idx_out)) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    const McfHostImage& im = h->im;
    *count = 0;
    if (im.m == 0) return MCF_OK;
    const int64_t nb = (im.m + kBnChunk - 1) / kBnChunk;
    int rc = lazy_group(h, "bottleneck scratch", {{&h->d_bn_flag, (size_t)im.m}, {&h->d_bn_cnt, (size_t)nb}, {&h->d_bn_off, (size_t)nb + 1}});
    if (rc) return rc;
    const int64_t want = idx_cap < im.m ? idx_cap : im.m;
    if (want > h->bn_idx_cap) {   // (sized to the request: never more than m entries)
        lazy_release({{&h->d_bn_idx, 0}});
        h->bn_idx_cap = 0;
        if ((rc = lazy_group(h, "bottleneck indices", {{&h->d_bn_idx, (size_t)want}})) != MCF_OK) return rc;
        h->bn_idx_cap = want;
    }
    const int64_t* cflow = nullptr;
    if ((rc = cert_upload_flow(h, flow, &cflow)) != MCF_OK) return rc;
    hipStream_t s = h->stream;
    int64_t fb = (im.m + kCertThreads - 1) / kCertThreads;
    if (fb > kCertMaxBlocks) fb = kCertMaxBlocks;
    hipLaunchKernelGGL(k_bn_flag, dim3((unsigned)fb), dim3(kCertThreads), 0, s, h->view, cflow, num, den, h->d_bn_flag);
    hipLaunchKernelGGL(k_bn_count, dim3((unsigned)nb), dim3(kCertThreads), 0, s, h->d_bn_flag, im.m, h->d_bn_cnt);
    hipLaunchKernelGGL((k_scan_chunks<int32_t, int64_t>), dim3(1), dim3(1024), 0, s, (const int32_t*)h->d_bn_cnt, nb, h->d_bn_off, h->d_bn_off + nb);
    if (want > 0) hipLaunchKernelGGL(k_bn_write, dim3((unsigned)nb), dim3(kCertThreads), 0, s, h->d_bn_flag, im.m, h->d_bn_off, h->d_bn_idx, want);
    HIP_TRY(h, hipGetLastError());
    int64_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, h->d_bn_off + nb, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *count = total;
    const int64_t got = total < want ? total : want;
    if (got > 0) HIP_TRY(h, hipMemcpy(idx_out, h->d_bn_idx, (size_t)got * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

// ---- witnesses of the unbounded and the infeasible verdict (include/mcf.h)
int mcf_certify_ray(mcf_handle* h, int64_t arc, int64_t* idx_out, int64_t idx_cap, mcf_ray* out) {
    if (!h || !out || idx_cap < 0 || (idx_cap > 0 && !idx_out)) return MCF_E_BAD_ARG;
    const McfHostImage& im = h->im;
    if (arc < -1 || arc >= im.m) { h->err = "mcf_certify_ray: arc index outside [0, m)"; return MCF_E_BAD_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    int64_t e;
    if (arc < 0) {
        if (h->h_ctx->status != MCF_UNBOUNDED || h->h_ctx->unbounded_arc < 0 || h->h_ctx->unbounded_arc >= im.m) {
            h->err = "mcf_certify_ray: the handle's status is not unbounded"; return MCF_E_STATE;
        }
        e = h->h_ctx->unbounded_arc;
    } else {
        uc_index(h);
        e = h->uc_inv[(size_t)arc];
    }
    int8_t st = 0;
    HIP_TRY(h, hipMemcpy(&st, h->d_state + e, 1, hipMemcpyDeviceToHost));
    if (st == 0) { h->err = "mcf_certify_ray: the arc is basic"; return MCF_E_BAD_ARG; }
    const int32_t backward = st < 0 ? 1 : 0;
    if ((rc = lazy_group(h, "ray scratch", {{&h->d_ray_part, kCertMaxBlocks + 1}, {&h->d_ray_idx, (size_t)im.n_nodes}})) != MCF_OK) return rc;
    for (hipEvent_t& ev : h->ct_ev) if (!ev) HIP_TRY(h, hipEventCreate(&ev));
    CertArgs a;
    std::memset(&a, 0, sizeof a);
    a.pi = h->d_pi;
    a.cur = tree_sel(*h->h_ctx).cur;
    a.arena = tree_sel(*h->h_ctx).arena;
    a.bigm = im.big_m;
    const int nb = node_grid(im.n_nodes);
    const int64_t want = idx_cap < im.n_nodes ? idx_cap : im.n_nodes;   // a cycle has at most n + 1 = n_nodes arcs
    hipStream_t s = h->stream;
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
    hipLaunchKernelGGL(k_ray_nodes, dim3(nb), dim3(kCertThreads), 0, s, h->view, a, e, backward, h->d_ray_part);
    hipLaunchKernelGGL(k_final<McfRayAcc>, dim3(1), dim3(kCertThreads), 0, s, h->d_ray_part, nb);
    if (want > 0) hipLaunchKernelGGL(k_ray_write, dim3(nb), dim3(kCertThreads), 0, s, h->view, a, e, backward, h->d_ray_part + nb, h->d_ray_idx, want);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    HIP_TRY(h, hipGetLastError());
    McfRayAcc R;
    HIP_TRY(h, hipMemcpyAsync(&R, h->d_ray_part + nb, sizeof R, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ct_ev[0], h->ct_ev[1]));
    mcf_ray r;
    std::memset(&r, 0, sizeof r);
    r.arc = im.orig[e];
    r.entering_backward = backward;
    r.length = R.tree_n + 1;
    r.join = R.join_i == MCF_CERT_NONE ? -1 : R.join_i;
    r.backward_count = R.back_n; r.capped_count = R.cap_n; r.artificial_count = R.art_n;
    r.cost = R.cost; r.reduced_cost = R.rc;
    r.theta = R.theta; r.theta_arc = R.theta_i == MCF_CERT_NONE ? -1 : R.theta_i;
    r.proven = mcf_ray_proven(R, backward != 0) ? 1 : 0;
    r.device_ms = ms;
    const int64_t got = r.length < want ? r.length : want;
    if (got > 0) HIP_TRY(h, hipMemcpy(idx_out, h->d_ray_idx, (size_t)got * 8, hipMemcpyDeviceToHost));
    *out = r;
    return MCF_OK;
}

int mcf_certify_cut(mcf_handle* h, const int8_t* in_S, int8_t* S_out, mcf_cut* out) {
    if (!h || !out) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    const McfHostImage& im = h->im;
    if ((rc = cert_prepare(h, in_S == nullptr)) != MCF_OK) return rc;   // device supplies, events; a full adjacency for the search only
    if ((rc = lazy_group(h, "cut scratch", {{&h->d_cut_mark, (size_t)im.n}, {&h->d_cut_level, 1}, {&h->d_cut_byte, (size_t)im.n},
                                            {&h->d_cut_part, 2 * kCertMaxBlocks + 1}})) != MCF_OK) return rc;
    const FullAdj fa = full_adj(h);
    const int nb = node_grid(im.n);
    const int ab = mcf_price_blocks(im.m, 1, 0);
    hipStream_t s = h->stream;
    int32_t level = 0;
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
    if (in_S) {
        HIP_TRY(h, hipMemcpyAsync(h->d_cut_byte, in_S, (size_t)im.n, hipMemcpyHostToDevice, s));   // (the call ends with a synchronisation)
        hipLaunchKernelGGL(k_cut_widen, dim3(nb), dim3(kCertThreads), 0, s, h->d_cut_byte, im.n, h->d_cut_mark);
    } else {
        HIP_TRY(h, hipMemsetAsync(h->d_cut_level, 0, 4, s));
        hipLaunchKernelGGL(k_cut_seed, dim3(nb), dim3(kCertThreads), 0, s, h->view, h->d_cut_mark, h->d_cut_level);
        HIP_TRY(h, hipMemcpyAsync(&level, h->d_cut_level, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        // Round r expands level r and fills level r + 1; a level holds at least one new node, so there are at most n of them
        // and round n finds nothing new: the loop ends at r > n whatever the device arrays hold.
        int32_t r = 1;
        while (level > 0 && r <= im.n) {
            const int32_t stop = r + kCutBatch - 1 < im.n ? r + kCutBatch - 1 : im.n;
            for (; r <= stop; ++r) hipLaunchKernelGGL(k_cut_round, dim3(nb), dim3(kCertThreads), 0, s, h->view, fa.off, fa.adj, h->d_cut_mark, h->d_cut_level, r);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(&level, h->d_cut_level, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
            if (level < r) break;   // the last level was expanded (r is one past the rounds queued) and reached nothing new
        }
    }
    const int32_t resident = in_S ? 0 : 1;
    hipLaunchKernelGGL(im.m >= kIncrementalMinArcs ? k_cut_arcs<true> : k_cut_arcs<false>, dim3(ab), dim3(kCertThreads), 0, s, h->view, h->d_cut_mark, resident, h->d_cut_part);
    hipLaunchKernelGGL(k_cut_nodes, dim3(nb), dim3(kCertThreads), 0, s, h->view, h->d_cut_mark, h->d_ct_supply, resident, h->d_cut_part + ab);
    hipLaunchKernelGGL(k_final<McfCutAcc>, dim3(1), dim3(kCertThreads), 0, s, h->d_cut_part, ab + nb);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    HIP_TRY(h, hipGetLastError());
    McfCutAcc C;
    HIP_TRY(h, hipMemcpyAsync(&C, h->d_cut_part + ab + nb, sizeof C, hipMemcpyDeviceToHost, s));
    if (S_out) {
        hipLaunchKernelGGL(k_cut_narrow, dim3(nb), dim3(kCertThreads), 0, s, h->d_cut_mark, im.n, h->d_cut_byte);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(S_out, h->d_cut_byte, (size_t)im.n, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ct_ev[0], h->ct_ev[1]));
    mcf_cut c;
    std::memset(&c, 0, sizeof c);
    c.seeds = C.seeds; c.nodes_in_S = C.in_s; c.rounds = level; c.deficit_in_S = C.deficit;
    c.leaving_arcs = C.leave_n; c.leaving_uncapacitated = C.leave_uncap; c.leaving_unsaturated = C.leave_unsat; c.entering_with_flow = C.enter_flow;
    __int128 excess = 0;
    c.proven = mcf_cut_proven(C, &excess) ? 1 : 0;
    put128(c.capacity, (__int128)(((mcf_u128)C.cap_hi << 64) | C.cap_lo));
    put128(c.supply, (__int128)(((mcf_u128)C.sup_hi << 64) | C.sup_lo));
    put128(c.excess, excess);
    put128(c.artificial_out, (__int128)(((mcf_u128)C.art_hi << 64) | C.art_lo));
    c.device_ms = ms;
    *out = c;
    return MCF_OK;
}

}  // extern "C"
