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

// ---- mcf_update_rhs_dual: the dual phase (kernels k_dual_* / k_pivot_dual).  The first census has run with `keep`, the
// control block on the host is current.  Pivots are queued in batches of kDualBatch; one DualState record comes back per batch.
constexpr int kDualBatch = 32;
// enter_walk = 0: walk the adjacency of subtrees up to this many nodes.  A guess, bounded by what was measured at 262 144 /
// 2 097 152 (profiles/update_rhs_dual_262k_2m.txt): walking up to 4 096 nodes costs 144.7 us per dual pivot against 139.8 us with
// the sweep alone, walking every subtree 145 us per search against the sweep's 34 us; with the walk up to 64 nodes 5 995 of 223 893
// pivots walk and the time per pivot is the same (140.3 us); neither search was timed on its own at that size.
constexpr int kDualWalkAuto = 64;
// max_pivots < 0: this many pivots per violation of the first census -- twice the largest ratio measured (81.45 dual pivots per
// violation, supplies edit of the same profile)
constexpr int64_t kDualBudgetMul = 163;
constexpr int64_t kDualBudgetMax = (int64_t)1 << 60;   // no budget is larger

int dual_phase(mcf_handle* h, const FullAdj& fa, const mcf_dual_options* dopt, int64_t* log, int64_t log_cap, int64_t violations,
               mcf_dual_report* drep) {
    const McfHostImage& im = h->im;
    hipStream_t s = h->stream;
    int rc;
    const int ab = mcf_price_blocks(im.m, 1, 0), nb = node_grid(im.n_nodes);
    if ((rc = lazy_group(h, "dual pivot partials", {{&h->d_dual_leave, (size_t)kCertMaxBlocks + 1}, {&h->d_dual_enter, (size_t)kMaxPriceBlocks},
                                                    {&h->d_dual_state, 1}, {&h->d_dual_count, 1}})) != MCF_OK) return rc;
    // dual feasibility: one census over the arcs
    const bool nt = im.m >= kIncrementalMinArcs;
    HIP_TRY(h, hipMemsetAsync(h->d_dual_count, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(nt ? k_dual_census<true> : k_dual_census<false>, dim3(ab), dim3(kPassThreads), 0, s, h->view, h->d_dual_count);
    HIP_TRY(h, hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(h, hipMemcpyAsync(&bad, h->d_dual_count, sizeof bad, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (bad > 0) { drep->reason = 3; return MCF_OK; }

    int64_t budget = dopt && dopt->max_pivots >= 0 ? dopt->max_pivots : kDualBudgetMul * violations;
    if (budget > kDualBudgetMax) budget = kDualBudgetMax;   // (the loop below counts past it in steps of kDualBatch)
    const int32_t ew = dopt ? dopt->enter_walk : 0;
    const int64_t keep_log = log_cap < budget ? log_cap : budget;
    if ((rc = lazy_grow(h, "dual pivot log", &h->dual_log_cap, keep_log, {{&h->d_dual_log, 4}})) != MCF_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(h, hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(ev[0]); h->err = "hipEventCreate"; return MCF_E_HIP; }
    const McfCtx was = *h->h_ctx;
    // every way out after this point: the events go, and the host's control block says what it said before
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(s); (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); (void)hipGetLastError();
        h->h_ctx->status = was.status;
        h->ctx_current = false;
        return code;
    };

    // the control block says "running" for the pivot machinery (as every path of the call leaves it in the end)
    h->h_ctx->status = MCF_RUNNING;
    DualState st;
    std::memset(&st, 0, sizeof st);
    st.max_pivots = budget;
    if (hipMemcpyAsync(h->d_ctx, h->h_ctx, sizeof(McfCtx), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(h->d_dual_state, &st, sizeof st, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipEventRecord(ev[0], s) != hipSuccess) { h->err = "mcf_update_rhs_dual: upload"; return fail(MCF_E_HIP); }
    h->ctx_current = false;
    DualArgs a;
    a.ctx = h->d_ctx;
    a.leave = h->d_dual_leave + nb;
    a.st = h->d_dual_state;
    a.adj_off = fa.off; a.adj = fa.adj;
    a.walk_max = ew < 0 ? 0 : (ew == 0 ? kDualWalkAuto : ew);
    // MCF_DUAL_TIMING=1 (diagnostic, like MCF_STAMPS): HIP events round the launches of every pivot, one line on stderr at the
    // end -- where a dual pivot's time goes.  The pivots are then synchronised one by one.
    const char* tenv = std::getenv("MCF_DUAL_TIMING");
    const bool timing = tenv && tenv[0] == '1';
    hipEvent_t tev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double tms[4] = {0, 0, 0, 0};
    int64_t timed = 0;
    if (timing) for (hipEvent_t& x : tev) if (hipEventCreate(&x) != hipSuccess) { (void)hipGetLastError(); x = nullptr; }
    const bool tim = timing && tev[4] != nullptr;
    // every pivot the budget allows plus the one launch that finds nothing left: bounded in code, whatever the device reports
    for (int64_t queued = 0; queued <= budget; queued += kDualBatch) {
        for (int i = 0; i < kDualBatch; ++i) {
            if (tim) (void)hipEventRecord(tev[0], s);
            hipLaunchKernelGGL(k_dual_leave, dim3(nb), dim3(kPassThreads), 0, s, h->view, (const DualState*)h->d_dual_state, h->d_dual_leave);
            hipLaunchKernelGGL(k_final<McfDualLeave>, dim3(1), dim3(kPassThreads), 0, s, h->d_dual_leave, nb);
            if (tim) (void)hipEventRecord(tev[1], s);
            hipLaunchKernelGGL(nt ? k_dual_enter<true> : k_dual_enter<false>, dim3(ab), dim3(kPassThreads), 0, s, h->view, a, h->d_dual_enter);
            if (tim) (void)hipEventRecord(tev[2], s);
            if (h->bpl) hipLaunchKernelGGL(k_pivot_dual<true>, dim3(1), dim3(kPivotThreads), 0, s, h->view, a, (const McfDualEnter*)h->d_dual_enter, ab, h->d_dual_state, h->d_dual_log, keep_log);
            else hipLaunchKernelGGL(k_pivot_dual<false>, dim3(1), dim3(kPivotThreads), 0, s, h->view, a, (const McfDualEnter*)h->d_dual_enter, ab, h->d_dual_state, h->d_dual_log, keep_log);
            if (tim) (void)hipEventRecord(tev[3], s);
            launch_apply(h, s);
            if (tim) {
                (void)hipEventRecord(tev[4], s);
                if (hipEventSynchronize(tev[4]) == hipSuccess) {
                    for (int k = 0; k < 4; ++k) { float ms1 = 0; if (hipEventElapsedTime(&ms1, tev[k], tev[k + 1]) == hipSuccess) tms[k] += ms1; }
                    ++timed;
                }
                (void)hipGetLastError();
            }
        }
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&st, h->d_dual_state, sizeof st, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { for (hipEvent_t x : tev) if (x) (void)hipEventDestroy(x); h->err = "mcf_update_rhs_dual: pivot batch"; return fail(MCF_E_HIP); }
        if (st.status != DUAL_RUNNING) break;
    }
    for (hipEvent_t x : tev) if (x) (void)hipEventDestroy(x);
    if (tim && timed > 0)
        std::fprintf(stderr, "mcf_update_rhs_dual timing: %lld pivot slots (%lld pivots: %lld sweeps, %lld walks), us per slot: leave %.2f, enter %.2f, "
                     "pivot %.2f, update %.2f\n", (long long)timed, (long long)st.pivots, (long long)st.sweeps, (long long)st.walks,
                     tms[0] * 1e3 / timed, tms[1] * 1e3 / timed, tms[2] * 1e3 / timed, tms[3] * 1e3 / timed);
    {   // closed arcs take the state their reduced cost asks for (key codes only where they are kept exact)
        McfView vw = h->view;
        if (!h->rcached) vw.vkey = nullptr;
        hipLaunchKernelGGL(nt ? k_dual_close<true> : k_dual_close<false>, dim3(ab), dim3(kPassThreads), 0, s, vw);
    }
    if (hipEventRecord(ev[1], s) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess) { h->err = "mcf_update_rhs_dual: events"; return fail(MCF_E_HIP); }
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
    drep->device_ms = ms;
    drep->dual_pivots = st.pivots;
    drep->sweeps = st.sweeps;
    drep->walks = st.walks;
    drep->log_written = st.pivots < keep_log ? st.pivots : keep_log;
    if (drep->log_written > 0 && hipMemcpy(log, h->d_dual_log, (size_t)drep->log_written * 4 * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) {
        h->err = "mcf_update_rhs_dual: log download"; return fail(MCF_E_HIP);
    }
    if ((rc = read_ctx(h, s)) != MCF_OK) return fail(rc);
    (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
    if (st.status == DUAL_INTERNAL || h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "mcf_update_rhs_dual: the dual pivot passes disagree (internal error)"; return MCF_E_STATE; }
    // the solver's counters do not move in the phase: its work is in the report
    McfCtx& c = *h->h_ctx;
    c.status = was.status;
    c.pivots = was.pivots; c.degenerate = was.degenerate; c.bound_flips = was.bound_flips; c.arcs_priced = was.arcs_priced;
    c.nodes_moved = was.nodes_moved; c.subtree_nodes = was.subtree_nodes; c.cycle_arcs = was.cycle_arcs;
    c.scans = was.scans; c.scan_rounds = was.scan_rounds; c.rebuilds = was.rebuilds;
    HIP_TRY(h, hipMemcpyAsync(h->d_ctx, h->h_ctx, sizeof(McfCtx), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->ctx_current = true;
    drep->ended = st.status == DUAL_CLEARED ? 0 : st.status == DUAL_NO_ENTERING ? 1 : st.status == DUAL_MAGNITUDE ? 4 : 2;
    drep->reason = 0;
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
// (mcf_update_rhs_dual is this very call with a dual simplex phase between two runs of the census: `dual`)
static int rhs_update(mcf_handle* h, int64_t n_sup, const int64_t* node, const int64_t* new_supply, int64_t n_cap,
                      const int64_t* arc, const int64_t* new_cap, mcf_rhs_report* out, bool dual, const mcf_dual_options* dopt,
                      int64_t* log, int64_t log_cap, mcf_dual_report* dual_out) {
    if (!h) return MCF_E_BAD_ARG;
    if (dual && (log_cap < 0 || (log_cap > 0 && !log))) { h->err = "mcf_update_rhs_dual: bad log_cap / null log"; return MCF_E_BAD_ARG; }
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
    unsigned long long info[RHS_COUNTERS] = {0, 0, 0, 0, 0};
    int32_t depth[2] = {0, 0};
    // the passes up to the census (`scatter`: with the edit itself; `cur`: the copy of the preorder arrays that is current;
    // `keep`: violating tree flows are stored too), and its figures on the host
    auto census = [&](bool scatter, int32_t cur, int32_t keep) -> int {
        HIP_TRY(h, hipMemsetAsync(h->d_rhs_info, 0, RHS_COUNTERS * sizeof(unsigned long long), s));
        HIP_TRY(h, hipMemsetAsync(h->d_uc_info, 0, 2 * sizeof(int32_t), s));
        HIP_TRY(h, hipMemsetAsync(h->d_rhs_bal, 0, (size_t)N * sizeof(mcf_u128), s));
        if (scatter && ns + nc > 0)
            hipLaunchKernelGGL(k_rhs_scatter, dim3(uc_blocks_for(ns > nc ? ns : nc)), dim3(kRhsThreads), 0, s, vw, ns, (const int32_t*)h->d_rhs_idx,
                               (const int64_t*)h->d_rhs_val, h->d_ct_supply, nc, (const int32_t*)(h->d_rhs_idx + ns), (const int64_t*)(h->d_rhs_val + ns), h->d_rhs_info);
        hipLaunchKernelGGL(k_rhs_balance, dim3(uc_blocks_for(N)), dim3(kRhsThreads), 0, s, vw, cur, (const int64_t*)h->d_ct_supply,
                           fa.off, fa.adj, h->d_rhs_bal);
        hipLaunchKernelGGL(k_rhs_scan_totals, dim3((unsigned)chunks), dim3(kRhsThreads), 0, s, (const mcf_u128*)h->d_rhs_bal, N, h->d_rhs_part);
        hipLaunchKernelGGL((k_scan_chunks<mcf_u128, mcf_u128>), dim3(1), dim3(1024), 0, s, (const mcf_u128*)h->d_rhs_part, chunks, h->d_rhs_part, (mcf_u128*)nullptr);
        hipLaunchKernelGGL(k_rhs_scan_apply, dim3((unsigned)chunks), dim3(kRhsThreads), 0, s, h->d_rhs_bal, N, (const mcf_u128*)h->d_rhs_part);
        // jump records for the potentials below an artificial arc that turns round (seeded with 0; the flow pass marks the turns)
        hipLaunchKernelGGL(k_uc_seed, dim3(uc_blocks_for(N)), dim3(kUcThreads), 0, s, (const McfNode*)h->d_node, N, im.m, (int64_t)0, h->d_uc_jump[0], h->d_uc_info);
        hipLaunchKernelGGL(k_rhs_flows, dim3(uc_blocks_for(N)), dim3(kRhsThreads), 0, s, vw, cur, (const mcf_u128*)h->d_rhs_bal, im.big_m, h->d_uc_jump[0], h->d_rhs_info, keep);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(info, h->d_rhs_info, sizeof info, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(depth, h->d_uc_info, sizeof depth, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));   // (also: the pageable sources above are free again)
        return MCF_OK;
    };
    if ((rc = census(true, cur, dual ? 1 : 0)) != MCF_OK) return rc;

    // host image: the objective, a later mcf_reset / mcf_set_basis and the repair below use the new data
    for (int64_t i = 0; i < ns; ++i) im.supply[(size_t)idx[(size_t)i]] = val[(size_t)i];
    for (int64_t i = ns; i < ns + nc; ++i) im.arcw[(size_t)idx[(size_t)i]].cap = val[(size_t)i];

    mcf_rhs_report rep;
    std::memset(&rep, 0, sizeof rep);
    rep.tree_violations = (int64_t)info[RHS_VIOL];
    rep.wrong_way = (int64_t)info[RHS_WRONG];
    rep.art_flips = (int64_t)info[RHS_FLIPS];
    rep.upper_moved = (int64_t)info[RHS_MOVED];
    if (dual) {
        mcf_dual_report drep;
        std::memset(&drep, 0, sizeof drep);
        drep.violations_before = drep.violations_after = rep.tree_violations;
        drep.wrong_way_after = rep.wrong_way;
        drep.ended = 3;
        if (rep.tree_violations == 0) drep.reason = 1;
        else if (h->small || h->mid) drep.reason = 2;
        else if (rep.art_flips > 0) drep.reason = 4;
        else if (info[RHS_HUGE] > 0) drep.reason = 5;
        else if ((rc = dual_phase(h, fa, dopt, log, log_cap, rep.tree_violations, &drep)) != MCF_OK) return rc;
        if (drep.ended != 3) {
            // the phase ran: tree flows and census once more, on the basis it left
            const int64_t moved = rep.upper_moved;
            if ((rc = census(false, tree_sel(*h->h_ctx).cur, 0)) != MCF_OK) return rc;
            std::memset(&rep, 0, sizeof rep);
            rep.tree_violations = (int64_t)info[RHS_VIOL];
            rep.wrong_way = (int64_t)info[RHS_WRONG];
            rep.art_flips = (int64_t)info[RHS_FLIPS];
            rep.upper_moved = moved;
            drep.violations_after = rep.tree_violations;
            drep.wrong_way_after = rep.wrong_way;
        }
        if (dual_out) *dual_out = drep;
    }
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

int mcf_update_rhs(mcf_handle* h, int64_t n_sup, const int64_t* node, const int64_t* new_supply, int64_t n_cap,
                   const int64_t* arc, const int64_t* new_cap, mcf_rhs_report* out) {
    return rhs_update(h, n_sup, node, new_supply, n_cap, arc, new_cap, out, false, nullptr, nullptr, 0, nullptr);
}

int mcf_update_rhs_dual(mcf_handle* h, int64_t n_sup, const int64_t* node, const int64_t* new_supply, int64_t n_cap,
                        const int64_t* arc, const int64_t* new_cap, const mcf_dual_options* opt, int64_t* log, int64_t log_cap,
                        mcf_rhs_report* out, mcf_dual_report* dual_out) {
    return rhs_update(h, n_sup, node, new_supply, n_cap, arc, new_cap, out, true, opt, log, log_cap, dual_out);
}

// Add arcs to the resident handle (kernels k_aa_* above).  The new arcs are sorted on the host and uploaded with their keys
// and the sorted list of their end points; the re-layout of everything the handle holds per arc runs on the device, out of
// place, and the pointers are swapped once every pass has completed.  Everything is validated before the first byte moves.
int mcf_add_arcs(mcf_handle* h, int64_t count, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                 const int8_t* arc_priority, mcf_arcs_report* out) {
    if (!h) return MCF_E_BAD_ARG;
    if (h->shards != 1) {
        h->err = "mcf_add_arcs: handle was created with shard_count > 1; sharded handles cannot change their topology";
        return MCF_E_STATE;
    }
    if (count < 0 || (count > 0 && (!tail || !head || !cost || !cap))) { h->err = "mcf_add_arcs: bad count / null array"; return MCF_E_BAD_ARG; }
    McfHostImage& im = h->im;
    const int64_t k = count, m = im.m, m2 = m + k;
    const int32_t n = im.n, N = im.n_nodes;
    // (on the count alone, before an array is read)
    if (k >= ((int64_t)1 << 30) || (int64_t)n + m2 >= ((int64_t)1 << 30)) { h->err = "mcf_add_arcs: m + count + n must stay below 2^30"; return MCF_E_RANGE; }
    for (int64_t i = 0; i < k; ++i) {
        if (tail[i] < 0 || tail[i] >= n || head[i] < 0 || head[i] >= n) { h->err = "mcf_add_arcs: arc end point out of range"; return MCF_E_BAD_ARG; }
        if (tail[i] == head[i]) { h->err = "mcf_add_arcs: self-loop"; return MCF_E_BAD_ARG; }
    }
    int64_t max_abs = 0;
    for (int64_t i = 0; i < k; ++i) {
        if (cost[i] > INT32_MAX || cost[i] < -(int64_t)INT32_MAX) { h->err = "mcf_add_arcs: |cost| must fit int32"; return MCF_E_RANGE; }
        const int64_t a = cost[i] < 0 ? -cost[i] : cost[i];
        if (a > max_abs) max_abs = a;
    }
    // big-M never shrinks; it grows when a new cost needs it (same rule as mcf_build_image)
    int64_t big_m = im.big_m;
    if ((max_abs + 1) * ((int64_t)n + 2) > big_m) big_m = (max_abs + 1) * ((int64_t)n + 2);
    if (big_m >= ((int64_t)1 << 44)) { h->err = "mcf_add_arcs: max|cost| * n too large for big-M"; return MCF_E_RANGE; }
    const int64_t d_bigm = big_m - im.big_m;
    const int64_t m_pad2 = m2 > 0 ? ((m2 + 1023) / 1024) * 1024 : 1024;
    // the handle keeps its engine path: the fused LDS loop has to hold the grown instance
    SmallLayout L2 = h->small_layout;
    if (h->small && k > 0 && !small_plan(m_pad2, (size_t)(m2 + n), N, h->opt.rule == MCF_RULE_DEVEX_BLOCK, &L2)) {
        h->err = "mcf_add_arcs: the grown instance exceeds the LDS capacity of the fused small-instance loop (k_solve_small) this handle runs on";
        return MCF_E_STATE;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->small && k > 0 && !small_reserve(h->device, L2.total)) {
        h->err = "mcf_add_arcs: the device refuses the dynamic LDS the grown instance needs in the fused small-instance loop (k_solve_small)";
        return MCF_E_STATE;
    }
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    if (h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "mcf_add_arcs: the handle's tree is not usable"; return MCF_E_STATE; }
    if (d_bigm != 0 && (rc = uc_alloc(h)) != MCF_OK) return rc;
    for (hipEvent_t& ev : h->ct_ev) if (!ev) HIP_TRY(h, hipEventCreate(&ev));
    hipStream_t s = h->stream;
    mcf_arcs_report rep;
    std::memset(&rep, 0, sizeof rep);
    rep.first_index = m;
    rep.m = m2;

    // ---- the new arcs in engine order: (head bucket, tail, given order)
    const int64_t per = mcf_topo_per(n);
    std::vector<int64_t> perm((size_t)k);
    for (int64_t i = 0; i < k; ++i) perm[(size_t)i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return mcf_topo_key(tail[a], head[a], per) < mcf_topo_key(tail[b], head[b], per); });
    std::vector<int64_t> nkey((size_t)k), ncap((size_t)k);
    std::vector<int32_t> ntail((size_t)k), nhead((size_t)k), ncost((size_t)k), norig((size_t)k);
    std::vector<int8_t> nprio((size_t)k, 0);
    for (int64_t r = 0; r < k; ++r) {
        const int64_t i = perm[(size_t)r];
        nkey[(size_t)r] = mcf_topo_key(tail[i], head[i], per);
        ntail[(size_t)r] = tail[i]; nhead[(size_t)r] = head[i]; ncost[(size_t)r] = (int32_t)cost[i]; norig[(size_t)r] = (int32_t)(m + i);
        ncap[(size_t)r] = (cap[i] < 0 || cap[i] >= MCF_INF) ? MCF_INF : cap[i];
        if (arc_priority) nprio[(size_t)r] = (int8_t)(arc_priority[i] & 3);
    }
    // ... and their 2k end points sorted by node (the handle's adjacency, where it holds one)
    const bool with_adj = h->d_adj != nullptr;
    const int64_t k2 = with_adj ? 2 * k : 0;
    std::vector<int64_t> ep_node((size_t)k2), ep_end((size_t)k2), ep_val((size_t)k2);
    if (with_adj) {
        std::vector<int64_t> ep((size_t)k2);   // (node << 32) | (rank << 1) | is-tail: sorts by node, then rank
        for (int64_t r = 0; r < k; ++r) {
            ep[(size_t)(2 * r)] = ((int64_t)ntail[(size_t)r] << 32) | (r << 1) | 1;
            ep[(size_t)(2 * r + 1)] = ((int64_t)nhead[(size_t)r] << 32) | (r << 1);
        }
        std::sort(ep.begin(), ep.end());
        for (int64_t j = 0; j < k2; ++j) {
            const int64_t u = ep[(size_t)j] >> 32, r = (ep[(size_t)j] & 0xffffffffll) >> 1, is_tail = ep[(size_t)j] & 1;
            ep_node[(size_t)j] = u;
            ep_end[(size_t)j] = im.adj_off[(size_t)u + 1];
            ep_val[(size_t)j] = ((int64_t)(is_tail ? nhead[(size_t)r] : ntail[(size_t)r]) << 32) | (r << 1) | is_tail;
        }
    }

    if (k == 0) {   // nothing to lay out: the tail of an empty mcf_update_costs
        HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
        if ((rc = uc_finish(h, true)) != MCF_OK) return rc;
        HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
        HIP_TRY(h, hipEventSynchronize(h->ct_ev[1]));
        float ms0 = 0;
        if (hipEventElapsedTime(&ms0, h->ct_ev[0], h->ct_ev[1]) != hipSuccess) { (void)hipGetLastError(); ms0 = 0; }
        rep.device_ms = ms0;
        if (out) *out = rep;
        return MCF_OK;
    }

    // ---- device memory: the upload buffers (freed on return) and the new arrays (the handle's once every pass has completed)
    std::vector<void*> temps;
    struct Fresh { void** field; void* ptr; size_t bytes; };
    std::vector<Fresh> fresh;
    auto give_up = [&](int code, const char* what) {
        (void)hipStreamSynchronize(s);
        for (void* p : temps) (void)hipFree(p);
        for (const Fresh& f : fresh) (void)hipFree(f.ptr);
        (void)hipGetLastError();
        if (what) h->err = std::string("mcf_add_arcs: ") + what;
        return code;
    };
    bool alloc_ok = true;
    auto temp = [&](auto** p, size_t cnt) {
        *p = nullptr;
        if (!alloc_ok) return;
        if (dalloc(p, cnt) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; alloc_ok = false; return; }
        temps.push_back(*p);
    };
    auto renew = [&](auto** field, auto** p, size_t cnt) {   // a new array for *field (skipped where the handle has none)
        *p = nullptr;
        if (!alloc_ok || !*field) return;
        if (dalloc(p, cnt) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; alloc_ok = false; return; }
        fresh.push_back({reinterpret_cast<void**>(field), *p, cnt * sizeof(**p)});
    };
    int64_t *t_nkey, *t_ncap, *t_npos, *t_epn, *t_epe, *t_epv;
    int32_t *t_ntail, *t_nhead, *t_ncost, *t_norig, *t_emap;
    int8_t* t_nprio;
    unsigned long long* t_info;
    temp(&t_nkey, (size_t)k); temp(&t_ncap, (size_t)k); temp(&t_npos, (size_t)k);
    temp(&t_epn, (size_t)k2); temp(&t_epe, (size_t)k2); temp(&t_epv, (size_t)k2);
    temp(&t_ntail, (size_t)k); temp(&t_nhead, (size_t)k); temp(&t_ncost, (size_t)k); temp(&t_norig, (size_t)k); temp(&t_emap, (size_t)m);
    temp(&t_nprio, (size_t)k); temp(&t_info, 2);
    int32_t *x_tail, *x_head, *x_cost, *x_orig, *x_vkey;
    int8_t *x_state, *x_prio;
    float* x_weight;
    McfArcW* x_arcw;
    McfNode* x_node;
    int64_t *x_rcache, *x_adj_off, *x_adj;
    renew(&h->d_tail, &x_tail, (size_t)m_pad2); renew(&h->d_head, &x_head, (size_t)m_pad2);
    renew(&h->d_cost, &x_cost, (size_t)m_pad2); renew(&h->d_orig, &x_orig, (size_t)m_pad2);
    renew(&h->d_state, &x_state, (size_t)m_pad2); renew(&h->d_prio, &x_prio, (size_t)m_pad2);
    renew(&h->d_weight, &x_weight, (size_t)m_pad2); renew(&h->d_arcw, &x_arcw, (size_t)(m2 + n));
    renew(&h->d_node, &x_node, (size_t)N);
    renew(&h->d_rcache, &x_rcache, (size_t)m_pad2); renew(&h->d_vkey, &x_vkey, (size_t)m_pad2);
    renew(&h->d_adj_off, &x_adj_off, (size_t)n + 1); renew(&h->d_adj, &x_adj, (size_t)(2 * m2));
    if (!alloc_ok) return give_up(MCF_E_ALLOC, "hipMalloc of the new arc arrays (the arc arrays exist twice for the duration of the call)");

    // ---- device passes, part one: everything that does not touch what the handle holds
    auto hip_ok = [&](hipError_t e) { return e == hipSuccess; };
    bool ok = hip_ok(hipEventRecord(h->ct_ev[0], s));
    auto up = [&](void* dst, const void* src, size_t bytes) { if (ok && bytes) ok = hip_ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)); };
    up(t_nkey, nkey.data(), (size_t)k * 8); up(t_ncap, ncap.data(), (size_t)k * 8);
    up(t_ntail, ntail.data(), (size_t)k * 4); up(t_nhead, nhead.data(), (size_t)k * 4);
    up(t_ncost, ncost.data(), (size_t)k * 4); up(t_norig, norig.data(), (size_t)k * 4); up(t_nprio, nprio.data(), (size_t)k);
    up(t_epn, ep_node.data(), (size_t)k2 * 8); up(t_epe, ep_end.data(), (size_t)k2 * 8); up(t_epv, ep_val.data(), (size_t)k2 * 8);
    if (ok) ok = hip_ok(hipMemsetAsync(t_info, 0, 2 * sizeof(unsigned long long), s));
    // padding arcs [m2, m_pad2): zeros, state 0
    const size_t padn = (size_t)(m_pad2 - m2);
    auto zero = [&](void* base, size_t elem) { if (ok && base && padn) ok = hip_ok(hipMemsetAsync((char*)base + (size_t)m2 * elem, 0, padn * elem, s)); };
    zero(x_tail, 4); zero(x_head, 4); zero(x_cost, 4); zero(x_orig, 4); zero(x_state, 1); zero(x_prio, 1); zero(x_rcache, 8); zero(x_vkey, 4);
    if (!ok) return give_up(MCF_E_HIP, "upload of the new arcs");
    AaArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = m; a.k = k; a.per = per;
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) a.bucket_off[x] = im.bucket_off[x];
    a.nkey = t_nkey; a.ntail = t_ntail; a.nhead = t_nhead; a.ncost = t_ncost; a.norig = t_norig; a.ncap = t_ncap;
    a.nprio = arc_priority ? t_nprio : nullptr; a.npos = t_npos;
    a.tail = h->d_tail; a.head = h->d_head; a.cost = h->d_cost; a.orig = h->d_orig; a.state = h->d_state; a.prio = h->d_prio;
    a.rcache = h->d_rcache; a.vkey = h->d_vkey; a.arcw = h->d_arcw;
    a.tail2 = x_tail; a.head2 = x_head; a.cost2 = x_cost; a.orig2 = x_orig; a.state2 = x_state; a.prio2 = x_prio;
    a.rcache2 = x_rcache; a.vkey2 = x_vkey; a.arcw2 = x_arcw;
    a.emap = t_emap; a.info = t_info;
    hipLaunchKernelGGL(k_aa_new, dim3(uc_blocks_for(k)), dim3(kAaThreads), 0, s, a);
    if (m > 0) {
        const int64_t chunks = (m + kAaChunk - 1) / kAaChunk;
        const unsigned grid = (unsigned)(chunks < 4096 ? chunks : 4096);
        hipLaunchKernelGGL(m >= kIncrementalMinArcs ? k_aa_scatter<true> : k_aa_scatter<false>, dim3(grid), dim3(kAaThreads), 0, s, a);
    }
    hipLaunchKernelGGL(k_uc_ones, dim3(uc_blocks_for(m_pad2 / 4)), dim3(kUcThreads), 0, s, reinterpret_cast<float4*>(x_weight), m_pad2 / 4);
    ok = hip_ok(hipMemcpyAsync(x_arcw + m2, h->d_arcw + m, (size_t)n * sizeof(McfArcW), hipMemcpyDeviceToDevice, s));   // the artificial block, shifted by k
    hipLaunchKernelGGL(k_aa_nodes, dim3(uc_blocks_for(N)), dim3(kAaThreads), 0, s, (const McfNode*)h->d_node, N, m, k, (const int32_t*)t_emap, x_node);
    if (with_adj) {
        hipLaunchKernelGGL(k_aa_adj_off, dim3(uc_blocks_for((int64_t)n + 1)), dim3(kAaThreads), 0, s, (const int64_t*)h->d_adj_off, (int64_t)n + 1, (const int64_t*)t_epn, k2, x_adj_off);
        if (m > 0) hipLaunchKernelGGL(k_aa_adj, dim3(uc_blocks_for(2 * m)), dim3(kAaThreads), 0, s, (const int64_t*)h->d_adj, 2 * m, (const int64_t*)t_epe, k2, (const int32_t*)t_emap, x_adj);
        hipLaunchKernelGGL(k_aa_adj_new, dim3(uc_blocks_for(k2)), dim3(kAaThreads), 0, s, (const int64_t*)t_epv, (const int64_t*)t_epe, k2, (const int64_t*)t_npos, x_adj);
    }
    if (!ok || hipGetLastError() != hipSuccess) return give_up(MCF_E_HIP, "launch of the re-layout passes");
    // device_ms brackets stream work only: this pair closes behind the last re-layout pass, a second pair goes round part two
    unsigned long long info[2] = {0, 0};
    if (hipEventRecord(h->ct_ev[1], s) != hipSuccess || hipMemcpyAsync(info, t_info, sizeof info, hipMemcpyDeviceToHost, s) != hipSuccess)
        return give_up(MCF_E_HIP, "launch of the re-layout passes");

    // ---- the host image's own merge, while the device works: host work outside both event pairs.  The indices come from the
    // same counting rules the kernels use (mcf_core.h).  Everything that can fail for lack of memory -- the extended image,
    // the header of the incremental sweeps, the Devex granule table -- is built here, before anything changes.
    McfHostImage nim;
    std::vector<int32_t> emap_h((size_t)m);
    std::vector<McfDirty> dirty_head;   // 0 or 1 entry
    std::vector<McfDevex> granules;     // 0 or 1 entry
    try {
        nim.tail.assign((size_t)m_pad2, 0); nim.head.assign((size_t)m_pad2, 0); nim.cost.assign((size_t)m_pad2, 0); nim.orig.assign((size_t)m_pad2, 0);
        nim.cost64.assign((size_t)m2, 0); nim.state.assign((size_t)m_pad2, 0); nim.weight.assign((size_t)m_pad2, 1.0f);
        nim.arcw.assign((size_t)(m2 + n), McfArcW{0, 0});
        if (!im.rcache.empty()) nim.rcache.assign((size_t)m_pad2, 0);
        for (int64_t e = 0; e < m; ++e) {
            const size_t d = (size_t)mcf_topo_old_index(e, mcf_topo_key(im.tail[(size_t)e], im.head[(size_t)e], per), nkey.data(), k);
            emap_h[(size_t)e] = (int32_t)d;
            nim.tail[d] = im.tail[(size_t)e]; nim.head[d] = im.head[(size_t)e]; nim.cost[d] = im.cost[(size_t)e]; nim.orig[d] = im.orig[(size_t)e];
            nim.cost64[d] = im.cost64[(size_t)e]; nim.state[d] = im.state[(size_t)e]; nim.arcw[d] = im.arcw[(size_t)e];
            if (!nim.rcache.empty()) nim.rcache[d] = im.rcache[(size_t)e];
        }
        for (int64_t r = 0; r < k; ++r) {
            const size_t d = (size_t)mcf_topo_new_index(r, nkey[(size_t)r], im.tail.data(), im.bucket_off);
            nim.tail[d] = ntail[(size_t)r]; nim.head[d] = nhead[(size_t)r]; nim.cost[d] = ncost[(size_t)r]; nim.orig[d] = norig[(size_t)r];
            nim.cost64[d] = ncost[(size_t)r]; nim.state[d] = 1; nim.arcw[d] = McfArcW{ncap[(size_t)r], 0};
            // (nim.rcache[d] stays 0: the image's potentials are those of the last upload, and mcf_reset / mcf_set_basis refresh
            //  every reduced cost of the image before they use one)
        }
        for (int32_t v = 0; v < n; ++v) nim.arcw[(size_t)(m2 + v)] = im.arcw[(size_t)(m + v)];
        if (!im.adj_off.empty()) {
            nim.adj_off.assign((size_t)n + 1, 0);
            for (int32_t u = 0; u <= n; ++u) nim.adj_off[(size_t)u] = mcf_topo_adj_off(im.adj_off[(size_t)u], u, ep_node.data(), k2);
        }
        for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) nim.bucket_off[x] = im.bucket_off[x] + mcf_count_below(nkey.data(), k, (int64_t)x << 32);
        if (h->d_dirty) {   // the header of the incremental sweeps: this rank's share of every bucket
            dirty_head.resize(1);
            dirty_head[0].nlb = h->price_blocks / MCF_NUM_BUCKETS;
            for (int x = 0; x < MCF_NUM_BUCKETS; ++x) { dirty_head[0].lo[x] = (int32_t)nim.bucket_off[x]; dirty_head[0].hi[x] = (int32_t)nim.bucket_off[x + 1]; }
        }
        if (h->d_dx) {      // Devex: the granule table of the new bucket ranges
            granules.resize(1);
            std::memset(&granules[0], 0, sizeof(McfDevex));
            mcf_devex_fill_granules(&granules[0], nim.bucket_off);
        }
    } catch (const std::bad_alloc&) {
        return give_up(MCF_E_ALLOC, "host allocation of the extended image");
    }
    if (hipStreamSynchronize(s) != hipSuccess) return give_up(MCF_E_HIP, "the re-layout passes failed");
    float ms1 = 0, ms2 = 0;
    if (hipEventElapsedTime(&ms1, h->ct_ev[0], h->ct_ev[1]) != hipSuccess) { (void)hipGetLastError(); ms1 = 0; }
    rep.shifted_only = (int64_t)info[0];

    // ---- every pass has completed: the handle takes the new arrays over (the old ones are freed at the end: a free synchronises)
    std::vector<void*> old_arrays;
    for (const Fresh& f : fresh) {
        old_arrays.push_back(*f.field); *f.field = f.ptr;
        for (mcf_handle::DevArray& a : h->arrays) if (a.field == f.field) a.bytes = f.bytes;   // (what mcf_fork copies and mcf_restore compares)
    }
    fresh.clear();
    McfView& v = h->view;
    v.m = m2;
    v.tail = h->d_tail; v.head = h->d_head; v.cost = h->d_cost; v.orig = h->d_orig; v.state = h->d_state;
    if (v.weight) v.weight = h->d_weight;
    if (v.prio) v.prio = h->d_prio;
    v.arcw = h->d_arcw; v.node = h->d_node;
    if (v.rcache) v.rcache = h->d_rcache;
    if (v.vkey) v.vkey = h->d_vkey;
    if (v.adj) { v.adj = h->d_adj; v.adj_off = h->d_adj_off; }
    v.vk_bigm = big_m;
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) v.bucket_off[x] = nim.bucket_off[x];
    for (int32_t u = 0; u < N; ++u) {   // the image's node records follow (a later mcf_reset / mcf_set_basis rewrites them anyway)
        int32_t& pred = im.node[(size_t)u].pred;
        if (pred < 0) continue;
        const int64_t arc = pred >> 1;
        pred = (int32_t)(((arc >= m ? arc + k : (int64_t)emap_h[(size_t)arc]) << 1) | (pred & 1));
    }
    im.tail.swap(nim.tail); im.head.swap(nim.head); im.cost.swap(nim.cost); im.orig.swap(nim.orig); im.cost64.swap(nim.cost64);
    im.state.swap(nim.state); im.weight.swap(nim.weight); im.arcw.swap(nim.arcw);
    if (!im.rcache.empty()) im.rcache.swap(nim.rcache);
    if (!im.adj_off.empty()) im.adj_off.swap(nim.adj_off);
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) im.bucket_off[x] = nim.bucket_off[x];
    im.m = m2; im.m_pad = m_pad2; im.big_m = big_m;
    if (h->small) h->small_layout = L2;
    h->shape = shape_of(h);
    drop_graph(h);   // (captured graphs carry the view by value)
    h->uc_inv.clear(); h->uc_stamp.clear();   // (rebuilt for the new m on their next use)
    // ---- device passes, part two (its own event pair): the small tables, potentials when big-M grew, the new arcs' reduced
    // costs, the tail of mcf_update_costs.  A failure from here on is MCF_E_HIP and leaves the handle unusable (include/mcf.h).
    ok = hip_ok(hipEventRecord(h->ct_ev[0], s));
    if (ok && !dirty_head.empty()) ok = hip_ok(hipMemcpyAsync(h->d_dirty, dirty_head.data(), offsetof(McfDirty, flag), hipMemcpyHostToDevice, s));
    if (ok && !granules.empty()) ok = hip_ok(hipMemcpyAsync(h->d_dx, granules.data(), offsetof(McfDevex, wlist), hipMemcpyHostToDevice, s));
    if (ok && d_bigm != 0) {
        int32_t depth[2] = {0, 0};
        ok = hip_ok(hipMemsetAsync(h->d_uc_info, 0, 2 * sizeof(int32_t), s));
        hipLaunchKernelGGL(k_uc_seed, dim3(uc_blocks_for(N)), dim3(kUcThreads), 0, s, (const McfNode*)h->d_node, N, m2, d_bigm, h->d_uc_jump[0], h->d_uc_info);
        if (ok) ok = hip_ok(hipMemcpyAsync(depth, h->d_uc_info, sizeof depth, hipMemcpyDeviceToHost, s));
        if (ok) ok = hip_ok(hipStreamSynchronize(s));   // (the depth of the tree decides the number of jump rounds)
        if (ok) uc_jump_rounds(h, depth[0]);
        rep.bigm_grew = 1;
    }
    if (ok) {
        hipLaunchKernelGGL(k_aa_price, dim3(uc_blocks_for(k)), dim3(kAaThreads), 0, s, h->view, (const int64_t*)t_npos, k,
                           h->rcached ? h->d_rcache : (int64_t*)nullptr, h->rcached ? h->view.vkey : (int32_t*)nullptr, t_info);
        ok = hip_ok(hipGetLastError());
    }
    if (ok) ok = hip_ok(hipMemcpyAsync(info, t_info, sizeof info, hipMemcpyDeviceToHost, s));
    rc = ok ? uc_finish(h, d_bigm != 0) : MCF_E_HIP;   // (ends with a synchronisation of the stream)
    if (rc == MCF_OK && (hipEventRecord(h->ct_ev[1], s) != hipSuccess || hipEventSynchronize(h->ct_ev[1]) != hipSuccess)) rc = MCF_E_HIP;
    if (rc != MCF_OK) (void)hipStreamSynchronize(s);
    // scratch of this call, the old arrays, and the other passes' scratch whose size depends on m (allocated again on its next use)
    for (void* p : temps) (void)hipFree(p);
    temps.clear();
    for (void* p : old_arrays) (void)hipFree(p);
    lazy_release({{&h->d_ct_flow, 0}, {&h->d_ct_adj_off, 0}, {&h->d_ct_adj, 0}, {&h->d_bn_flag, 0}, {&h->d_bn_cnt, 0}, {&h->d_bn_off, 0}});
    if (rc != MCF_OK) {
        (void)hipGetLastError();
        if (!ok) h->err = "mcf_add_arcs: a device pass after the re-layout failed; the handle is no longer usable";
        return rc;
    }
    if (hipEventElapsedTime(&ms2, h->ct_ev[0], h->ct_ev[1]) != hipSuccess) { (void)hipGetLastError(); ms2 = 0; }
    // per-pass accounting follows the grown shard (as upload_image sets it)
    h->shard_arcs = im.m;
    h->priced_per_pass = h->opt.rule == MCF_RULE_DEVEX_BLOCK ? h->shard_arcs * h->h_ctx->block_granules / MCF_GRANULES : h->shard_arcs;
    {
        const bool devex = h->opt.rule == MCF_RULE_DEVEX_BLOCK;
        if (h->d_vkey && !devex) h->stats.price_bytes = 4 * h->priced_per_pass;
        else if (h->rcached) h->stats.price_bytes = (devex ? 13 : 9) * h->priced_per_pass;
        else h->stats.price_bytes = (devex ? 17 : 13) * h->priced_per_pass + 8 * (int64_t)im.n_nodes;
    }
    rep.eligible = (int64_t)info[1];
    rep.device_ms = ms1 + ms2;
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

// ---- what cost ranging and flow ranging share: the greatest depth, which decides the number of levels (one word comes back
// before the tables are sized; *ms: the device time of the pass), and the ancestors with the two 8-byte tables
static int rng_max_depth(mcf_handle* h, McfRngDepthAcc* D, float* ms) {
    int rc;
    if ((rc = lazy_group(h, "ranging partials", {{&h->d_rng_part, kCertMaxBlocks + 1}, {&h->d_rng_info, (size_t)RNG_COUNTERS}})) != MCF_OK) return rc;
    for (hipEvent_t& ev : h->ct_ev) if (!ev) HIP_TRY(h, hipEventCreate(&ev));
    const int32_t N = h->im.n_nodes;
    const int nb = node_grid(N);
    hipStream_t s = h->stream;
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
    hipLaunchKernelGGL(k_rng_depth, dim3(nb), dim3(kRngThreads), 0, s, (const McfNode*)h->d_node, N, h->d_rng_part);
    hipLaunchKernelGGL(k_final<McfRngDepthAcc>, dim3(1), dim3(kPassThreads), 0, s, h->d_rng_part, nb);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(D, h->d_rng_part + nb, sizeof *D, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ct_ev[0], h->ct_ev[1]));
    return MCF_OK;
}
// released and allocated again when the levels outgrew them
static int rng_tables(mcf_handle* h, int64_t cells) {
    if (cells <= h->rng_cells) return MCF_OK;
    lazy_release({{&h->d_rng_anc, 0}, {&h->d_rng_p, 0}, {&h->d_rng_n, 0}});
    h->rng_cells = 0;
    const int rc = lazy_alloc(h, "ranging tables", {{&h->d_rng_anc, 1}, {&h->d_rng_p, 1}, {&h->d_rng_n, 1}}, (size_t)cells);
    if (rc == MCF_OK) h->rng_cells = cells;
    return rc;
}

// ---- cost ranging on the resident basis (include/mcf.h; kernels k_rng_* above, logic mcf_core.h: mcf_rng_*)
int mcf_cost_ranges(mcf_handle* h, int64_t count, const int64_t* arc, int64_t* down, int64_t* up, mcf_ranges_report* out) {
    if (!h) return MCF_E_BAD_ARG;
    const McfHostImage& im = h->im;
    const bool all = count < 0;
    if (all ? arc != nullptr : (count > 0 && !arc)) { h->err = "mcf_cost_ranges: count < 0 goes with a null index list, count > 0 with one"; return MCF_E_BAD_ARG; }
    const int64_t entries = all ? im.m : count;
    if (entries > 0 && (!down || !up)) { h->err = "mcf_cost_ranges: null output array"; return MCF_E_BAD_ARG; }
    for (int64_t i = 0; !all && i < count; ++i)
        if (arc[i] < 0 || arc[i] >= im.m) { h->err = "mcf_cost_ranges: arc index outside [0, m)"; return MCF_E_BAD_ARG; }
    mcf_ranges_report rep;
    std::memset(&rep, 0, sizeof rep);
    rep.big_m = im.big_m;
    if (im.m == 0 || im.n <= 1) {   // nothing to range: an empty answer
        rep.basic_artificial = im.n;
        rep.levels = 1;
        rep.max_depth = im.n > 0 ? 1 : 0;
        if (out) *out = rep;
        return MCF_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    const int32_t N = im.n_nodes;
    const int nb = node_grid(N);
    hipStream_t s = h->stream;
    McfRngDepthAcc D;
    float ms1 = 0, ms2 = 0;
    if ((rc = rng_max_depth(h, &D, &ms1)) != MCF_OK) return rc;
    const int K = mcf_rng_levels(D.depth);

    // ---- scratch: the tables, the answer (released and allocated again when m outgrew it: mcf_add_arcs), the list
    if ((rc = rng_tables(h, (int64_t)K * N)) != MCF_OK) return rc;
    if (im.m > h->rng_arcs) {
        lazy_release({{&h->d_rng_down, 0}, {&h->d_rng_up, 0}});
        h->rng_arcs = 0;
        if ((rc = lazy_alloc(h, "ranges", {{&h->d_rng_down, 1}, {&h->d_rng_up, 1}}, (size_t)im.m)) != MCF_OK) return rc;
        h->rng_arcs = im.m;
    }
    if (!all && (rc = lazy_grow(h, "range indices", &h->rng_list, count, {{&h->d_rng_idx, 1}, {&h->d_rng_gdown, 1}, {&h->d_rng_gup, 1}})) != MCF_OK) return rc;

    RngArgs a;
    std::memset(&a, 0, sizeof a);
    a.K = K;
    a.count_inf = all ? 1 : 0;
    a.anc = h->d_rng_anc; a.tab[0] = h->d_rng_p; a.tab[1] = h->d_rng_n;
    a.down = h->d_rng_down; a.up = h->d_rng_up;
    a.info = h->d_rng_info;
    int ab = mcf_price_blocks(im.m, 1, 0);
    if (ab > kRngMaxBlocks) ab = kRngMaxBlocks;
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));
    if (!all && count > 0) HIP_TRY(h, hipMemcpyAsync(h->d_rng_idx, arc, (size_t)count * 8, hipMemcpyHostToDevice, s));   // (the call ends with a synchronisation)
    HIP_TRY(h, hipMemsetAsync(h->d_rng_info, 0, RNG_COUNTERS * sizeof(unsigned long long), s));
    for (int k = 0; k < K; ++k) hipLaunchKernelGGL(k_rng_anc, dim3(nb), dim3(kRngThreads), 0, s, (const McfNode*)h->d_node, N, k, a);
    hipLaunchKernelGGL(k_rng_arcs, dim3(ab), dim3(kRngThreads), 0, s, h->view, a);
    for (int k = K - 1; k >= 1; --k) hipLaunchKernelGGL(k_rng_push, dim3(nb), dim3(kRngThreads), 0, s, N, k, a);
    hipLaunchKernelGGL(k_rng_out, dim3(nb), dim3(kRngThreads), 0, s, h->view, a);
    if (!all && count > 0)
        hipLaunchKernelGGL(k_rng_gather, dim3(uc_blocks_for(count)), dim3(kRngThreads), 0, s, count, (const int64_t*)h->d_rng_idx, (const int64_t*)h->d_rng_down,
                           (const int64_t*)h->d_rng_up, h->d_rng_gdown, h->d_rng_gup, h->d_rng_info);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    HIP_TRY(h, hipGetLastError());
    unsigned long long info[RNG_COUNTERS] = {0, 0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(info, h->d_rng_info, sizeof info, hipMemcpyDeviceToHost, s));
    if (entries > 0) {
        HIP_TRY(h, hipMemcpyAsync(down, all ? h->d_rng_down : h->d_rng_gdown, (size_t)entries * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(up, all ? h->d_rng_up : h->d_rng_gup, (size_t)entries * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, hipEventElapsedTime(&ms2, h->ct_ev[0], h->ct_ev[1]));
    rep.basic_real = (int64_t)info[RNG_BASIC_REAL];
    rep.basic_artificial = (int64_t)info[RNG_BASIC_ART];
    rep.eligible = (int64_t)info[RNG_ELIGIBLE];
    rep.max_depth = D.depth;
    rep.levels = K;
    rep.inf_down = (int64_t)info[RNG_INF_DOWN];
    rep.inf_up = (int64_t)info[RNG_INF_UP];
    rep.device_ms = ms1 + ms2;
    if (out) *out = rep;
    return MCF_OK;
}

// ---- flow ranging on the resident basis (include/mcf.h; kernels k_frng_* above, logic mcf_core.h: mcf_frng_*)
// Everything the two calls share up to their query pass: the levels, the scratch of the tables, and -- enqueued behind the
// event ct_ev[0] -- the counters, level 0 and the levels above it.
static int frng_tables(mcf_handle* h, FrngArgs* a, McfRngDepthAcc* D, float* ms_depth) {
    int rc;
    if ((rc = rng_max_depth(h, D, ms_depth)) != MCF_OK) return rc;
    const int32_t N = h->im.n_nodes;
    const int K = mcf_rng_levels(D->depth);
    const int64_t cells = (int64_t)K * N;
    if ((rc = rng_tables(h, cells)) != MCF_OK) return rc;
    if (cells > h->frng_cells) {
        lazy_release({{&h->d_frng_uid, 0}, {&h->d_frng_did, 0}});
        h->frng_cells = 0;
        if ((rc = lazy_alloc(h, "flow ranging tables", {{&h->d_frng_uid, 1}, {&h->d_frng_did, 1}}, (size_t)cells)) != MCF_OK) return rc;
        h->frng_cells = cells;
    }
    if ((rc = lazy_group(h, "flow ranging counters", {{&h->d_frng_info, (size_t)FRNG_COUNTERS}})) != MCF_OK) return rc;
    std::memset(a, 0, sizeof *a);
    a->K = K;
    a->anc = h->d_rng_anc;
    a->val[0] = h->d_rng_p; a->val[1] = h->d_rng_n;
    a->id[0] = h->d_frng_uid; a->id[1] = h->d_frng_did;
    a->info = h->d_frng_info;
    return MCF_OK;
}
static int frng_build(mcf_handle* h, const FrngArgs& a) {
    const int32_t N = h->im.n_nodes;
    const int nb = node_grid(N);
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemsetAsync(h->d_frng_info, 0, FRNG_COUNTERS * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_frng_base, dim3(nb), dim3(kFrngThreads), 0, s, h->view, a);
    for (int k = 1; k < a.K; ++k) hipLaunchKernelGGL(k_frng_level, dim3(nb), dim3(kFrngThreads), 0, s, N, k, a);
    return MCF_OK;
}
static void frng_report(mcf_flow_ranges_report* rep, const unsigned long long* info, const McfRngDepthAcc& D, int K, double ms) {
    rep->basic_real = (int64_t)info[FRNG_BASIC_REAL];
    rep->basic_artificial = (int64_t)info[FRNG_BASIC_ART];
    rep->at_capacity = (int64_t)info[FRNG_AT_CAP];
    rep->max_depth = D.depth;
    rep->levels = K;
    rep->inf_count = (int64_t)info[FRNG_INF];
    rep->zero_count = (int64_t)info[FRNG_ZERO];
    rep->art_rising_count = (int64_t)info[FRNG_RISING];
    rep->device_ms = ms;
}
static void frng_empty_report(mcf_flow_ranges_report* rep, const McfHostImage& im) {
    std::memset(rep, 0, sizeof *rep);
    rep->big_m = im.big_m;
    rep->basic_artificial = im.n;
    rep->levels = 1;
    rep->max_depth = im.n > 0 ? 1 : 0;
}

int mcf_supply_ranges(mcf_handle* h, int64_t count, const int32_t* from, const int32_t* to, int64_t* limit, int64_t* limit_arc, int64_t* rate,
                      int32_t* art_rising, mcf_flow_ranges_report* out) {
    if (!h) return MCF_E_BAD_ARG;
    const McfHostImage& im = h->im;
    if (count < 0 || (count > 0 && (!from || !to))) { h->err = "mcf_supply_ranges: a negative count, or a positive one without both node lists"; return MCF_E_BAD_ARG; }
    for (int64_t i = 0; i < count; ++i)
        if (from[i] < 0 || from[i] >= im.n || to[i] < 0 || to[i] >= im.n) { h->err = "mcf_supply_ranges: node index outside [0, n)"; return MCF_E_BAD_ARG; }
    mcf_flow_ranges_report rep;
    frng_empty_report(&rep, im);
    if (count == 0 || im.n <= 1) {   // no pair, or only pairs of the one node with itself: nothing limits, nothing moves
        for (int64_t i = 0; i < count; ++i) {
            if (limit) limit[i] = MCF_RANGE_INF;
            if (limit_arc) limit_arc[i] = -1;
            if (rate) rate[i] = 0;
            if (art_rising) art_rising[i] = 0;
        }
        rep.inf_count = count;
        if (out) *out = rep;
        return MCF_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    FrngArgs a;
    McfRngDepthAcc D;
    float ms1 = 0, ms2 = 0;
    if ((rc = frng_tables(h, &a, &D, &ms1)) != MCF_OK) return rc;
    if ((rc = lazy_grow(h, "supply range pairs", &h->frng_pairs, count, {{&h->d_frng_pair, 2}, {&h->d_frng_rise, 1}, {&h->d_frng_pout, 3}})) != MCF_OK) return rc;
    hipStream_t s = h->stream;
    int32_t* d_from = h->d_frng_pair;
    int32_t* d_to = h->d_frng_pair + count;
    int64_t *d_limit = h->d_frng_pout, *d_arc = h->d_frng_pout + count, *d_rate = h->d_frng_pout + 2 * count;
    HIP_TRY(h, hipMemcpyAsync(d_from, from, (size_t)count * 4, hipMemcpyHostToDevice, s));   // (the call ends with a synchronisation)
    HIP_TRY(h, hipMemcpyAsync(d_to, to, (size_t)count * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));   // (after the uploads: device_ms is the passes alone)
    if ((rc = frng_build(h, a)) != MCF_OK) return rc;
    hipLaunchKernelGGL(k_frng_pairs, dim3(uc_blocks_for(count)), dim3(kFrngThreads), 0, s, h->view, a, count, (const int32_t*)d_from, (const int32_t*)d_to,
                       d_limit, d_arc, d_rate, h->d_frng_rise);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    HIP_TRY(h, hipGetLastError());
    unsigned long long info[FRNG_COUNTERS] = {0, 0, 0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(info, h->d_frng_info, sizeof info, hipMemcpyDeviceToHost, s));
    if (limit) HIP_TRY(h, hipMemcpyAsync(limit, d_limit, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    if (limit_arc) HIP_TRY(h, hipMemcpyAsync(limit_arc, d_arc, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    if (rate) HIP_TRY(h, hipMemcpyAsync(rate, d_rate, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    if (art_rising) HIP_TRY(h, hipMemcpyAsync(art_rising, h->d_frng_rise, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, hipEventElapsedTime(&ms2, h->ct_ev[0], h->ct_ev[1]));
    frng_report(&rep, info, D, a.K, ms1 + ms2);
    if (out) *out = rep;
    return MCF_OK;
}

int mcf_capacity_ranges(mcf_handle* h, int64_t count, const int64_t* arc, int64_t* down, int64_t* up, int64_t* down_arc, int64_t* up_arc, int64_t* rate,
                        mcf_flow_ranges_report* out) {
    if (!h) return MCF_E_BAD_ARG;
    const McfHostImage& im = h->im;
    const bool all = count < 0;
    if (all ? arc != nullptr : (count > 0 && !arc)) { h->err = "mcf_capacity_ranges: count < 0 goes with a null index list, count > 0 with one"; return MCF_E_BAD_ARG; }
    for (int64_t i = 0; !all && i < count; ++i)
        if (arc[i] < 0 || arc[i] >= im.m) { h->err = "mcf_capacity_ranges: arc index outside [0, m)"; return MCF_E_BAD_ARG; }
    const int64_t entries = all ? im.m : count;
    mcf_flow_ranges_report rep;
    frng_empty_report(&rep, im);
    if (im.m == 0 || im.n <= 1 || entries == 0) {   // nothing to range: an empty answer
        if (out) *out = rep;
        return MCF_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    FrngArgs a;
    McfRngDepthAcc D;
    float ms1 = 0, ms2 = 0;
    if ((rc = frng_tables(h, &a, &D, &ms1)) != MCF_OK) return rc;
    const int64_t m = im.m;
    if (m != h->frng_arcs) {   // (laid out as five rows of m: mcf_add_arcs changes the layout)
        lazy_release({{&h->d_frng_out, 0}});
        h->frng_arcs = 0;
        if ((rc = lazy_alloc(h, "capacity ranges", {{&h->d_frng_out, 5}}, (size_t)m)) != MCF_OK) return rc;
        h->frng_arcs = m;
    }
    if (!all && (rc = lazy_grow(h, "capacity range indices", &h->frng_list, count, {{&h->d_frng_idx, 1}, {&h->d_frng_gout, 5}})) != MCF_OK) return rc;
    a.count_sides = all ? 1 : 0;
    a.out = h->d_frng_out;
    hipStream_t s = h->stream;
    int ab = mcf_price_blocks(m, 1, 0);
    if (ab > kFrngMaxBlocks) ab = kFrngMaxBlocks;
    if (!all) HIP_TRY(h, hipMemcpyAsync(h->d_frng_idx, arc, (size_t)count * 8, hipMemcpyHostToDevice, s));   // (the call ends with a synchronisation)
    HIP_TRY(h, hipEventRecord(h->ct_ev[0], s));   // (after the upload: device_ms is the passes alone)
    if ((rc = frng_build(h, a)) != MCF_OK) return rc;
    hipLaunchKernelGGL(k_frng_arcs, dim3(ab), dim3(kFrngThreads), 0, s, h->view, a);
    if (!all)
        hipLaunchKernelGGL(k_frng_gather, dim3(uc_blocks_for(count)), dim3(kFrngThreads), 0, s, count, m, (const int64_t*)h->d_frng_idx, (const int64_t*)h->d_frng_out,
                           h->d_frng_gout, h->d_frng_info);
    HIP_TRY(h, hipEventRecord(h->ct_ev[1], s));
    HIP_TRY(h, hipGetLastError());
    unsigned long long info[FRNG_COUNTERS] = {0, 0, 0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(info, h->d_frng_info, sizeof info, hipMemcpyDeviceToHost, s));
    const int64_t* src = all ? h->d_frng_out : h->d_frng_gout;
    int64_t* const dst[5] = {down, up, down_arc, up_arc, rate};
    for (int r = 0; r < 5; ++r)
        if (dst[r]) HIP_TRY(h, hipMemcpyAsync(dst[r], src + (size_t)r * entries, (size_t)entries * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, hipEventElapsedTime(&ms2, h->ct_ev[0], h->ct_ev[1]));
    frng_report(&rep, info, D, a.K, ms1 + ms2);
    if (out) *out = rep;
    return MCF_OK;
}

}  // extern "C"
