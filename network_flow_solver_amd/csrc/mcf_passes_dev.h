// mcf_passes_dev.h -- kernels of the post-solve passes on a resident handle (host drivers: mcf_passes_host.h).  Not a header
// of its own: mcf_engine.hip includes it inside its anonymous namespace, after the pivot-path kernels.

// ------------------------------------------------------------------ mcf_update_costs: re-price a resident basis
// Flows, states and the tree do not depend on costs, so a cost change on a handle that holds a basis moves only the
// potentials below a changed TREE arc and, after them, the reduced costs / key codes.  Four kinds of launches, none of
// which depends on how many arcs changed or (beyond a logarithm) on the depth of the tree:
//   k_uc_seed     one lane per node: jump record {val = 0 (root children on an artificial arc: +-(growth of big-M)),
//                 anc = parent}, and the greatest depth of the tree (decides the number of jump rounds);
//   k_uc_scatter  one lane per changed arc: store cost[e]; a basic arc adds +-delta to the record of the end point it is
//                 the tree arc of (every node has its own tree arc: plain stores, nothing to resolve);
//   k_uc_jump     pointer jumping, ceil(log2(max depth)) rounds over double buffers: val[v] += val[anc[v]],
//                 anc[v] = anc[anc[v]] -- after the last round val[v] is the sum of the deltas on v's root path.  Reads
//                 parent pointers only, so it serves the dense preorder array and the blocked preorder list alike;
//                 the last round adds the sum to pi[v] itself;
//   k_uc_rebuild  one streaming pass over all m_pad arcs in the shape of k_price's gather: rc = cost + pi[tail] - pi[head]
//                 into rcache (and the key code into vkey), 16-byte accesses throughout.
struct alignas(16) McfJump {
    int64_t val;   // sum of the potential shifts of the tree arcs from this node up to (excluding) anc
    int32_t anc;   // -1: the path has reached the root
    int32_t pad;
};

constexpr int kUcThreads = 256;

__global__ __launch_bounds__(kUcThreads) void k_uc_seed(const McfNode* __restrict__ node, int32_t n_nodes, int64_t m, int64_t d_bigm,
                                                        McfJump* __restrict__ out, int32_t* __restrict__ info) {
    __shared__ int32_t s_depth;
    if (threadIdx.x == 0) s_depth = 0;
    __syncthreads();
    int32_t deepest = 0;
    const int32_t stride = (int32_t)(gridDim.x * kUcThreads);
    for (int32_t v = (int32_t)(blockIdx.x * kUcThreads + threadIdx.x); v < n_nodes; v += stride) {
        const McfNode r = node[v];
        McfJump j;
        j.val = 0; j.anc = r.parent; j.pad = 0;
        // an artificial arc costs big-M: a larger big-M is a cost change on the tree arc of every node that still hangs on one
        if (r.pred >= 0 && (int64_t)(r.pred >> 1) >= m) j.val = (r.pred & 1) ? -d_bigm : d_bigm;
        out[v] = j;
        deepest = r.depth > deepest ? r.depth : deepest;
    }
    atomicMax(&s_depth, deepest);
    __syncthreads();
    if (threadIdx.x == 0 && s_depth > 0) atomicMax(&info[0], s_depth);
}

__global__ __launch_bounds__(kUcThreads) void k_uc_scatter(int64_t count, const int32_t* __restrict__ arc, const int32_t* __restrict__ new_cost,
                                                           int32_t* __restrict__ cost, const int8_t* __restrict__ state,
                                                           const int32_t* __restrict__ tail, const int32_t* __restrict__ head,
                                                           const McfNode* __restrict__ node, McfJump* __restrict__ jump, int32_t* __restrict__ info) {
    const int64_t stride = (int64_t)gridDim.x * kUcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kUcThreads + threadIdx.x; i < count; i += stride) {
        const int32_t e = arc[i];
        const int64_t delta = (int64_t)new_cost[i] - (int64_t)cost[e];
        cost[e] = new_cost[i];
        if (delta == 0 || state[e] != 0) continue;
        // basic: the arc is the tree arc of exactly one of its end points; pi[x] = pi[parent] -+ cost (up / down)
        const int32_t t = tail[e], hd = head[e];
        const int32_t pt = node[t].pred, ph = node[hd].pred;
        int32_t x = -1;
        if (pt >= 0 && (pt >> 1) == e) x = t; else if (ph >= 0 && (ph >> 1) == e) x = hd;
        if (x < 0) continue;
        jump[x].val = x == t ? -delta : delta;
        atomicAdd(&info[1], 1);
    }
}

template <bool LAST>   // LAST: the sums are complete after this round and go straight into the potentials
__global__ __launch_bounds__(kUcThreads) void k_uc_jump(const McfJump* __restrict__ in, McfJump* __restrict__ out, int64_t* __restrict__ pi, int32_t n_nodes) {
    const int32_t stride = (int32_t)(gridDim.x * kUcThreads);
    for (int32_t v = (int32_t)(blockIdx.x * kUcThreads + threadIdx.x); v < n_nodes; v += stride) {
        McfJump a = in[v];
        if (a.anc >= 0) {
            const McfJump b = in[a.anc];
            a.val += b.val;
            a.anc = b.anc;
        }
        if (LAST) { if (a.val != 0) pi[v] += a.val; }
        else out[v] = a;
    }
}

// Bucket x's share of the 4-arc groups: a group that straddles a bucket boundary belongs to the lower bucket, the last
// bucket takes the padding.  Workgroup b sweeps bucket b % 8 like k_price, so that the head gathers of an XCD's workgroups
// stay inside one eighth of the potential array.
__device__ __forceinline__ int64_t uc_group_lo(const McfView& v, int x, int64_t ngroups) {
    if (x <= 0) return 0;
    if (x >= MCF_NUM_BUCKETS) return ngroups;
    return (v.bucket_off[x] + 3) >> 2;
}

constexpr int kUcUnroll = 2;   // 4-arc groups in flight per lane, as in k_price

__global__ __launch_bounds__(kUcThreads) void k_uc_rebuild(McfView v, int64_t m_pad) {
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t ngroups = m_pad >> 2;
    const int64_t g_lo = uc_group_lo(v, x, ngroups), g_hi = uc_group_lo(v, x + 1, ngroups);
    const int4* __restrict__ tail4 = reinterpret_cast<const int4*>(v.tail);
    const int4* __restrict__ head4 = reinterpret_cast<const int4*>(v.head);
    const int4* __restrict__ cost4 = reinterpret_cast<const int4*>(v.cost);
    const int32_t* __restrict__ state4 = reinterpret_cast<const int32_t*>(v.state);
    const int64_t* __restrict__ pi = v.pi;
    longlong2* __restrict__ rc2 = reinterpret_cast<longlong2*>(v.rcache);
    int4* __restrict__ vk4 = reinterpret_cast<int4*>(v.vkey);
    const int64_t bigm = v.vk_bigm;
    const int32_t half = v.vk_half;
    const int64_t stride = nlb * kUcThreads;
    for (int64_t g0 = g_lo + lb * kUcThreads + threadIdx.x; g0 < g_hi; g0 += stride * kUcUnroll) {
        int4 t[kUcUnroll], h[kUcUnroll], cc[kUcUnroll];
        int32_t st[kUcUnroll];
#pragma unroll
        for (int u = 0; u < kUcUnroll; ++u) {
            const int64_t g = g0 + u * stride;
            const int64_t gs = g < g_hi ? g : g_lo;   // clamp: the loads stay unconditional and in range
            t[u] = tail4[gs]; h[u] = head4[gs]; cc[u] = cost4[gs]; st[u] = state4[gs];
        }
        int64_t pt[kUcUnroll][4], ph[kUcUnroll][4];
#pragma unroll
        for (int u = 0; u < kUcUnroll; ++u) {
            pt[u][0] = pi[t[u].x]; pt[u][1] = pi[t[u].y]; pt[u][2] = pi[t[u].z]; pt[u][3] = pi[t[u].w];
            ph[u][0] = pi[h[u].x]; ph[u][1] = pi[h[u].y]; ph[u][2] = pi[h[u].z]; ph[u][3] = pi[h[u].w];
        }
#pragma unroll
        for (int u = 0; u < kUcUnroll; ++u) {
            const int64_t g = g0 + u * stride;
            if (g >= g_hi) continue;
            const int64_t r0 = (int64_t)cc[u].x + pt[u][0] - ph[u][0], r1 = (int64_t)cc[u].y + pt[u][1] - ph[u][1];
            const int64_t r2 = (int64_t)cc[u].z + pt[u][2] - ph[u][2], r3 = (int64_t)cc[u].w + pt[u][3] - ph[u][3];
            longlong2 a, b;
            a.x = r0; a.y = r1; b.x = r2; b.y = r3;
            rc2[2 * g] = a;
            rc2[2 * g + 1] = b;
            if (vk4) {
                const int32_t s = st[u];
                int4 k;
                k.x = mcf_vkey(-(int64_t)(int8_t)s * r0, bigm, half);
                k.y = mcf_vkey(-(int64_t)(int8_t)(s >> 8) * r1, bigm, half);
                k.z = mcf_vkey(-(int64_t)(int8_t)(s >> 16) * r2, bigm, half);
                k.w = mcf_vkey(-(int64_t)(int8_t)(s >> 24) * r3, bigm, half);
                vk4[g] = k;
            }
        }
    }
}

__global__ __launch_bounds__(kUcThreads) void k_uc_ones(float4* __restrict__ w4, int64_t n4) {
    const int64_t stride = (int64_t)gridDim.x * kUcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kUcThreads + threadIdx.x; i < n4; i += stride) w4[i] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
}

// ------------------------------------------------------------------ certificate (mcf_certify / mcf_bottlenecks)
// k_cert_arcs    ONE streaming pass over the arcs in engine order, workgroup b on head bucket b % 8 like the pricing sweeps
//                (the two potential gathers of an arc then stay inside one XCD's L2 share): tail, head, cost, orig (4 B
//                each), the walk record (cap, flow: 16 B), and for the resident groups state (1 B), reduced cost (8 B) and
//                key code (4 B) -- 32 B per arc for the primal / dual / objective groups, 45 B with everything.  Read once
//                per call: non-temporal loads from kIncrementalMinArcs arcs on, as for the key-code sweep.
// k_cert_child   size[v] added to csum[parent[v]] (integer atomics: the sum does not depend on their order).
// k_cert_nodes   one lane per node: conservation as a gather over the node's adjacency list (128-bit balance), the dual
//                objective's node term, the artificial arc, and the tree records (mcf_get_tree's view of them).
// k_cert_final   one workgroup merges the per-workgroup partials.
// Every partial combines by integer +, max or (max, lowest index) (mcf_core.h), so no merge order can change the result.
constexpr int kCertThreads = 256;
constexpr int kCertMaxBlocks = 2048;

struct CertArgs {
    const int64_t* cflow;     // caller's flows in the caller's order; nullptr = resident
    const int64_t* pi;        // [n_nodes] potentials, root included (resident, or the caller's with root = 0)
    const int64_t* supply;    // [n]
    const int64_t* adj_off;   // full node -> arc adjacency (the handle's, or the certificate's own)
    const int64_t* adj;
    const int64_t* rcache;    // resident copies to compare, nullptr = none
    const int32_t* vkey;
    int32_t* csum;            // [n_nodes] scratch: sum of the children's sizes
    uint32_t checks;
    int32_t resident_flow;
    int32_t cur, arena;       // which copies of the preorder arrays are current (mcf_get_tree)
    int32_t partial;          // resident reduced costs / key codes are exact on this rank's shard only
    int64_t shard, shards;
    int64_t bigm;
};

template <bool NT, typename T>
__device__ __forceinline__ T cert_ld(const T* p) { return NT ? __builtin_nontemporal_load(p) : *p; }

// ---- building blocks shared by the passes below (workgroups of kPassThreads = 4 waves)
constexpr int kPassThreads = 256;
constexpr int kPassWaves = kPassThreads / 64;
static_assert(kCertThreads == kPassThreads, "block_reduce / wave_block_sum are written for 4 waves");

// an accumulator of mcf_core.h (mcf_acc_init / mcf_acc_merge): the workgroup's partials into thread 0's acc
template <typename Acc>
__device__ __forceinline__ void block_reduce(Acc& acc, Acc* s_wave) {
    for (int off = 32; off > 0; off >>= 1) {
        Acc o;
        unsigned long long* po = reinterpret_cast<unsigned long long*>(&o);
        const unsigned long long* pa = reinterpret_cast<const unsigned long long*>(&acc);
#pragma unroll
        for (int k = 0; k < mcf_acc_words<Acc>(); ++k) po[k] = __shfl_down(pa[k], off, 64);
        if ((int)(threadIdx.x & 63) + off < 64) mcf_acc_merge(&acc, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kPassWaves; ++w) mcf_acc_merge(&acc, s_wave[w]);
}

// part[0 .. n) -> part[n], by one workgroup
template <typename Acc>
__device__ __forceinline__ void merge_partials(Acc* __restrict__ part, int n, Acc* s_wave) {
    Acc acc;
    mcf_acc_init(&acc);
    for (int i = threadIdx.x; i < n; i += kPassThreads) mcf_acc_merge(&acc, part[i]);
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[n] = acc;
}
template <typename Acc>
__global__ __launch_bounds__(kPassThreads) void k_final(Acc* __restrict__ part, int n) {
    __shared__ Acc s_wave[kPassWaves];
    merge_partials(part, n, s_wave);
}

// integer sums: lane 0 of every wave gets its wave's (lanes past a shuffle's end add what their neighbours hold) ...
__device__ __forceinline__ int32_t wave_sum(int32_t x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
__device__ __forceinline__ mcf_u128 wave_sum(mcf_u128 x) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t lo = __shfl_down((unsigned long long)(uint64_t)x, off, 64), hi = __shfl_down((unsigned long long)(uint64_t)(x >> 64), off, 64);
        x += ((mcf_u128)hi << 64) | lo;
    }
    return x;
}
// ... and thread 0 the workgroup's (s: one slot per wave)
template <typename T>
__device__ __forceinline__ T wave_block_sum(T x, T* s) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

// Exclusive scan of nb chunk totals by ONE workgroup of 1024 threads: out[b] = in[0] + .. + in[b - 1] (out may be in),
// *total = the sum of all of them when asked for.  Thread t owns `per` consecutive chunks; thread 0 scans the 1024 sums.
template <typename In, typename Out>
__device__ __forceinline__ void scan_chunk_totals(const In* in, int64_t nb, Out* out, Out* total, Out* s) {
    const int64_t per = (nb + 1023) / 1024, lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    Out sum = 0;
    for (int64_t b = lo; b < hi; ++b) sum += in[b];
    s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        Out run = 0;
        for (int k = 0; k < 1024; ++k) { const Out x = s[k]; s[k] = run; run += x; }
        if (total) *total = run;
    }
    __syncthreads();
    Out run = s[threadIdx.x];
    for (int64_t b = lo; b < hi; ++b) { const Out x = in[b]; out[b] = run; run += x; }
}
template <typename In, typename Out>
__global__ __launch_bounds__(1024) void k_scan_chunks(const In* in, int64_t nb, Out* out, Out* total) {
    __shared__ Out s[1024];
    scan_chunk_totals(in, nb, out, total, s);
}

// Preorder position of `node` and the slot that holds it, in the view mcf_get_tree reports (cur: the copy that is current,
// a flip the last update left pending already accounted for -- tree_sel); -1 when a record points outside its array.
__device__ __forceinline__ int32_t tree_pos(const McfView& v, int32_t cur, int32_t node, int32_t* slot) {
    if (MCF_HAS_BPL(v)) {
        const int32_t s = v.posbuf[0][node] & MCF_LOC_SLOT;
        const int32_t b = s >> v.blk_shift;
        *slot = s;
        if (b < 0 || b >= v.blk_cap) return -1;
        const int32_t base = (cur ? v.bmeta[1] : v.bmeta[0])[b].base;
        if (base == MCF_BLK_FREE) return -1;
        const int32_t p = base + (s & ((1 << v.blk_shift) - 1));
        return p < v.n_nodes ? p : -1;
    }
    const int32_t p = (cur ? v.posbuf[1] : v.posbuf[0])[node];
    *slot = p;
    return (p < 0 || p >= v.n_nodes) ? -1 : p;
}

// node u's artificial arc: does it point u -> root ("up")?  A non-basic one carries nothing and counts as up.
__device__ __forceinline__ bool art_flow_up(const McfView& v, int32_t u) {
    const int32_t pred = v.node[u].pred;
    return (int64_t)(pred >> 1) == v.m + u ? (pred & 1) != 0 : true;
}

template <bool NT>
__global__ __launch_bounds__(kCertThreads) void k_cert_arcs(McfView v, CertArgs a, McfCertArcAcc* __restrict__ part) {
    __shared__ McfCertArcAcc s_wave[kCertThreads / 64];
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
    int64_t own_lo = lo, own_hi = hi;
    if (a.partial) mcf_bucket_slice(v.bucket_off, x, a.shard, a.shards, 0, 1, &own_lo, &own_hi);
    const bool resident = (a.checks & (MCF_CERT_BASIS | MCF_CERT_PRICING)) != 0;
    McfCertArcAcc acc;
    mcf_acc_init(&acc);
    for (int64_t e = lo + lb * kCertThreads + threadIdx.x; e < hi; e += nlb * kCertThreads) {
        const int32_t t = cert_ld<NT>(v.tail + e), hd = cert_ld<NT>(v.head + e);
        const int64_t cost = cert_ld<NT>(v.cost + e);
        const int64_t o = cert_ld<NT>(v.orig + e);
        const int64_t* aw = reinterpret_cast<const int64_t*>(v.arcw + e);
        const int64_t cap = cert_ld<NT>(aw);
        const int64_t flow = a.cflow ? a.cflow[o] : cert_ld<NT>(aw + 1);
        const int64_t rc = cost + a.pi[t] - a.pi[hd];
        mcf_cert_arc(&acc, a.checks, o, cost, cap, flow, rc);
        if (resident) {
            const int32_t st = cert_ld<NT>(v.state + e);
            const bool own = e >= own_lo && e < own_hi;
            int64_t rres = 0;
            int32_t kres = 0;
            if (a.rcache && own) rres = cert_ld<NT>(a.rcache + e);
            if (a.vkey && own) kres = cert_ld<NT>(a.vkey + e);
            mcf_cert_arc_resident(&acc, a.checks, cap, flow, rc, st, a.rcache && own ? &rres : nullptr, a.vkey && own ? &kres : nullptr,
                                  v.vk_bigm, v.vk_half);
        }
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kCertThreads) void k_cert_child(McfView v, int32_t* __restrict__ csum) {
    const int32_t N = v.n_nodes;
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < N - 1; u += gridDim.x * kCertThreads) {
        const McfNode nd = v.node[u];
        if (nd.parent >= 0 && nd.parent < N) atomicAdd(&csum[nd.parent], nd.size);
    }
}

__global__ __launch_bounds__(kCertThreads) void k_cert_nodes(McfView v, CertArgs a, McfCertNodeAcc* __restrict__ part) {
    __shared__ McfCertNodeAcc s_wave[kCertThreads / 64];
    const int32_t N = v.n_nodes, root = N - 1;
    const int64_t m = v.m;
    const int32_t sel = MCF_HAS_BPL(v) ? a.arena : a.cur;
    const int32_t* ord = sel ? v.order[1] : v.order[0];
    const int32_t* psz = sel ? v.psz[1] : v.psz[0];
    const int64_t pi_root = a.pi[root];
    McfCertNodeAcc acc;
    mcf_acc_init(&acc);
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < N; u += gridDim.x * kCertThreads) {
        const McfNode nd = v.node[u];
        if (u < root) {
            const int64_t af = v.arcw[m + u].flow;
            mcf_cert_add128(&acc.art_lo, &acc.art_hi, (mcf_u128)(__int128)af);
            if (a.checks & MCF_CERT_CONSERVATION) {
                // 128 bits: a node may have 2^30 arcs of up to 2^63 each
                __int128 bal = a.supply[u];
                for (int64_t k = a.adj_off[u]; k < a.adj_off[u + 1]; ++k) {
                    const int64_t w = a.adj[k];
                    const int64_t e = (w & 0xffffffff) >> 1;
                    const int64_t f = a.cflow ? a.cflow[v.orig[e]] : v.arcw[e].flow;
                    bal += (w & 1) ? -(__int128)f : (__int128)f;
                }
                if (a.resident_flow) {   // the node's artificial arc: node -> root when "up" (a non-basic one carries nothing)
                    bal += art_flow_up(v, u) ? -(__int128)af : (__int128)af;
                }
                mcf_cert_node_balance(&acc, u, bal);
            }
            if (a.checks & MCF_CERT_OBJECTIVES)
                mcf_cert_add128(&acc.dnode_lo, &acc.dnode_hi, (mcf_u128)(-(__int128)(a.pi[u] - pi_root) * a.supply[u]));
        }
        if (!(a.checks & MCF_CERT_BASIS)) continue;
        bool bad = false;
        int32_t slot = 0;
        const int32_t pos = tree_pos(v, a.cur, u, &slot);
        if (pos < 0) bad = true;
        else {
            if (ord[slot] != u) bad = true;
            if (psz && psz[slot] != nd.size) bad = true;
        }
        if (nd.size != 1 + a.csum[u]) bad = true;
        if (u == root) {
            if (nd.parent != -1 || pos != 0 || nd.size != N || nd.depth != 0) bad = true;
        } else if (nd.parent < 0 || nd.parent >= N || nd.pred < 0) {
            bad = true;
        } else {
            const int32_t p = nd.parent;
            const McfNode pn = v.node[p];
            int32_t pslot = 0;
            const int32_t ppos = tree_pos(v, a.cur, p, &pslot);
            if (ppos < 0 || pos < 0 || !(ppos < pos && (int64_t)pos + nd.size <= (int64_t)ppos + pn.size)) bad = true;
            if (nd.depth != pn.depth + 1) bad = true;
            const int64_t arc = nd.pred >> 1;
            const bool up = (nd.pred & 1) != 0;
            if (arc < m) {
                const int32_t t = v.tail[arc], hd = v.head[arc];
                if (up ? (t != u || hd != p) : (hd != u || t != p)) bad = true;
                if (v.state[arc] != 0) bad = true;
                if ((int64_t)v.cost[arc] + a.pi[t] - a.pi[hd] != 0) ++acc.tree_rc_bad;
                const McfArcW w = v.arcw[arc];
                if ((up && w.cap < MCF_INF && w.flow == w.cap) || (!up && w.flow == 0)) ++acc.strong_bad;
            } else {
                if (arc != m + u || p != root) bad = true;
                if (a.bigm + (up ? a.pi[u] - pi_root : pi_root - a.pi[u]) != 0) ++acc.tree_rc_bad;
                if (!up && v.arcw[m + u].flow == 0) ++acc.strong_bad;
                ++acc.art_basic;
            }
        }
        if (bad) ++acc.shape_bad;
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// part[0 .. n) -> part[n] (arcs and nodes alike)
__global__ __launch_bounds__(kCertThreads) void k_cert_final(McfCertArcAcc* __restrict__ ap, int na, McfCertNodeAcc* __restrict__ np, int nn) {
    __shared__ McfCertArcAcc s_a[kPassWaves];
    __shared__ McfCertNodeAcc s_n[kPassWaves];
    merge_partials(ap, na, s_a);
    merge_partials(np, nn, s_n);
}

// ---- bottleneck arcs, compacted in ascending caller's index: flag per caller's index (scatter from the engine-order
// stream), count per chunk, exclusive scan of the chunk counts by one workgroup, write.
constexpr int kBnChunk = 4096;   // caller's indices per workgroup: 16 rounds of 256
__global__ __launch_bounds__(kCertThreads) void k_bn_flag(McfView v, const int64_t* __restrict__ cflow, int64_t num, int64_t den,
                                                          uint8_t* __restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * kCertThreads + threadIdx.x; e < v.m; e += (int64_t)gridDim.x * kCertThreads) {
        const McfArcW w = v.arcw[e];
        const int32_t o = v.orig[e];
        flag[o] = mcf_cert_bottleneck(w.cap, cflow ? cflow[o] : w.flow, num, den) ? 1 : 0;
    }
}
__global__ __launch_bounds__(kCertThreads) void k_bn_count(const uint8_t* __restrict__ flag, int64_t m, int32_t* __restrict__ cnt) {
    __shared__ int32_t s[kCertThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kBnChunk;
    int32_t c = 0;
    for (int r = 0; r < kBnChunk / kCertThreads; ++r) {
        const int64_t i = base + r * kCertThreads + threadIdx.x;
        if (i < m && flag[i]) ++c;
    }
    c = wave_block_sum(c, s);
    if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}
__global__ __launch_bounds__(kCertThreads) void k_bn_write(const uint8_t* __restrict__ flag, int64_t m, const int64_t* __restrict__ off,
                                                           int64_t* __restrict__ idx, int64_t idx_cap) {
    __shared__ int32_t s[kCertThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kBnChunk;
    int64_t run = off[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = 0; r < kBnChunk / kCertThreads; ++r) {
        const int64_t i = base + r * kCertThreads + threadIdx.x;
        const bool f = i < m && flag[i];
        const uint64_t mask = __ballot(f);
        if (lane == 0) s[wave] = __popcll(mask);
        __syncthreads();
        int64_t before = run;
        for (int w = 0; w < wave; ++w) before += s[w];
        const int64_t at = before + __popcll(mask & (((uint64_t)1 << lane) - 1));
        if (f && at < idx_cap) idx[at] = i;
        run += s[0] + s[1] + s[2] + s[3];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ witnesses (mcf_certify_ray / mcf_certify_cut)
// k_ray_nodes   one lane per node record (16 B) + its preorder position (4 B dense; 4 + 8 B blocked: slot, block base): the
//               interval test against the two end points says whether the node's tree arc is on the cycle and on which
//               side; only the <= length lanes that are read the arc's walk record (16 B), cost and caller's index.
// k_final       one workgroup merges the per-workgroup partials (ray and cut alike).
// k_ray_write   the same pass once more, now that the length is known: a node of the arriving side lands at
//               1 + depth[first] - depth[u], one of the leaving side at length - 1 - (depth[second] - depth[u]).  8 B per cycle arc out.
// k_cut_seed    one lane per node: node record + artificial walk record in, a 4 B level mark out (1 = seed, 0 = not reached).
// k_cut_round   round r: one lane per node reads its mark (4 B); the lanes at level r walk their adjacency list (8 B per entry +
//               the arc's 16 B walk record + the other end's mark) and mark what the residual arcs reach with r + 1.  Every list
//               is expanded in exactly one round; all lanes that reach a node in a round store the same value.
// k_cut_arcs    the streaming pass of k_cert_arcs: tail, head (4 B each), the walk record (16 B), two gathered marks.
// k_cut_nodes   one lane per node: mark, supply (8 B), node record and artificial walk record of the nodes of S.
constexpr int kCutBatch = 32;   // rounds queued between two looks at the level word

__global__ __launch_bounds__(kCertThreads) void k_ray_nodes(McfView v, CertArgs a, int64_t e, int32_t backward, McfRayAcc* __restrict__ part) {
    __shared__ McfRayAcc s_wave[kCertThreads / 64];
    const int32_t N = v.n_nodes;
    const int64_t m = v.m;
    const int32_t t = v.tail[e], hd = v.head[e];
    const int32_t first = backward ? t : hd, second = backward ? hd : t;
    int32_t slot = 0;
    const int32_t pf = tree_pos(v, a.cur, first, &slot), ps = tree_pos(v, a.cur, second, &slot);
    McfRayAcc acc;
    mcf_acc_init(&acc);
    if (pf >= 0 && ps >= 0) {
        for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < N; u += gridDim.x * kCertThreads) {
            const McfNode nd = v.node[u];
            const int32_t pu = tree_pos(v, a.cur, u, &slot);
            if (pu < 0) continue;
            const int side = mcf_ray_side(pu, nd.size, pf, ps);
            if (side == 3) mcf_cert_worst(&acc.join_d, &acc.join_i, (int64_t)nd.depth + 1, u);
            else if (side && nd.pred >= 0) {
                const int64_t arc = nd.pred >> 1;
                const bool up = (nd.pred & 1) != 0;
                const bool forward = side == 1 ? up : !up;
                if (arc < m) {
                    const McfArcW w = v.arcw[arc];
                    mcf_ray_arc(&acc, v.orig[arc], true, false, forward, v.cost[arc], w.cap, w.flow);
                } else if (arc < m + N - 1) {
                    mcf_ray_arc(&acc, arc, true, true, forward, a.bigm, MCF_INF, v.arcw[arc].flow);
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const McfArcW w = v.arcw[e];
        const int64_t cost = v.cost[e];
        mcf_ray_arc(&acc, v.orig[e], false, false, !backward, cost, w.cap, w.flow);
        const int64_t rc = cost + a.pi[t] - a.pi[hd];
        acc.rc = backward ? -rc : rc;
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kCertThreads) void k_ray_write(McfView v, CertArgs a, int64_t e, int32_t backward, const McfRayAcc* __restrict__ total,
                                                            int64_t* __restrict__ idx, int64_t idx_cap) {
    const int32_t N = v.n_nodes;
    const int64_t m = v.m;
    const int32_t t = v.tail[e], hd = v.head[e];
    const int32_t first = backward ? t : hd, second = backward ? hd : t;
    int32_t slot = 0;
    const int32_t pf = tree_pos(v, a.cur, first, &slot), ps = tree_pos(v, a.cur, second, &slot);
    const int64_t length = total->tree_n + 1;
    const int64_t df = v.node[first].depth, ds = v.node[second].depth;
    if (blockIdx.x == 0 && threadIdx.x == 0 && idx_cap > 0) idx[0] = v.orig[e];
    if (pf < 0 || ps < 0) return;
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < N; u += gridDim.x * kCertThreads) {
        const McfNode nd = v.node[u];
        const int32_t pu = tree_pos(v, a.cur, u, &slot);
        if (pu < 0 || nd.pred < 0) continue;
        const int side = mcf_ray_side(pu, nd.size, pf, ps);
        if (side != 1 && side != 2) continue;
        const int64_t arc = nd.pred >> 1;
        const int64_t at = side == 1 ? 1 + df - nd.depth : length - 1 - (ds - nd.depth);
        if (at >= 1 && at < idx_cap && at < length) idx[at] = arc < m ? (int64_t)v.orig[arc] : arc;
    }
}

// the flow of node u's artificial arc, > 0 towards the root, < 0 from it (a non-basic one carries nothing and counts as "up")
__device__ __forceinline__ int64_t cut_art(const McfView& v, int32_t u) {
    const int64_t af = v.arcw[v.m + u].flow;
    return art_flow_up(v, u) ? af : -af;
}

__global__ __launch_bounds__(kCertThreads) void k_cut_seed(McfView v, int32_t* __restrict__ mark, int32_t* __restrict__ level) {
    const int32_t n = v.n_nodes - 1;
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < n; u += gridDim.x * kCertThreads) {
        const bool seed = cut_art(v, u) > 0;
        mark[u] = seed ? 1 : 0;
        if (seed) *level = 1;
    }
}

// mark[] is read while other lanes store r + 1 into entries that hold 0: a lane sees 0 or r + 1 there, and either is right
__global__ __launch_bounds__(kCertThreads) void k_cut_round(McfView v, const int64_t* __restrict__ adj_off, const int64_t* __restrict__ adj,
                                                            int32_t* mark, int32_t* __restrict__ level, int32_t r) {
    const int32_t n = v.n_nodes - 1;
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < n; u += gridDim.x * kCertThreads) {
        if (mark[u] != r) continue;
        for (int64_t k = adj_off[u]; k < adj_off[u + 1]; ++k) {
            const int64_t w = adj[k];
            const int32_t other = (int32_t)(w >> 32);
            if (other < 0 || other >= n || mark[other] != 0) continue;
            const McfArcW aw = v.arcw[(w & 0xffffffff) >> 1];
            if (mcf_cut_extends((w & 1) != 0, aw.cap, aw.flow)) { mark[other] = r + 1; *level = r + 1; }
        }
    }
}

// the caller's set, one byte per node, into level marks (1 / 0) -- and the marks back into bytes for S_out
__global__ __launch_bounds__(kCertThreads) void k_cut_widen(const int8_t* __restrict__ in, int32_t n, int32_t* __restrict__ mark) {
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < n; u += gridDim.x * kCertThreads) mark[u] = in[u] != 0 ? 1 : 0;
}
__global__ __launch_bounds__(kCertThreads) void k_cut_narrow(const int32_t* __restrict__ mark, int32_t n, int8_t* __restrict__ out) {
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < n; u += gridDim.x * kCertThreads) out[u] = mark[u] != 0 ? 1 : 0;
}

template <bool NT>
__global__ __launch_bounds__(kCertThreads) void k_cut_arcs(McfView v, const int32_t* __restrict__ mark, int32_t resident, McfCutAcc* __restrict__ part) {
    __shared__ McfCutAcc s_wave[kCertThreads / 64];
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
    McfCutAcc acc;
    mcf_acc_init(&acc);
    for (int64_t e = lo + lb * kCertThreads + threadIdx.x; e < hi; e += nlb * kCertThreads) {
        const int32_t t = cert_ld<NT>(v.tail + e), hd = cert_ld<NT>(v.head + e);
        const bool tin = mark[t] != 0, hin = mark[hd] != 0;
        if (tin == hin) continue;
        const int64_t* aw = reinterpret_cast<const int64_t*>(v.arcw + e);
        mcf_cut_arc(&acc, tin, hin, cert_ld<NT>(aw), cert_ld<NT>(aw + 1), resident != 0);
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kCertThreads) void k_cut_nodes(McfView v, const int32_t* __restrict__ mark, const int64_t* __restrict__ supply, int32_t resident,
                                                            McfCutAcc* __restrict__ part) {
    __shared__ McfCutAcc s_wave[kCertThreads / 64];
    const int32_t n = v.n_nodes - 1;
    McfCutAcc acc;
    mcf_acc_init(&acc);
    for (int32_t u = blockIdx.x * kCertThreads + threadIdx.x; u < n; u += gridDim.x * kCertThreads)
        if (mark[u] != 0) mcf_cut_node(&acc, supply[u], resident ? cut_art(v, u) : 0);
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ------------------------------------------------------------------ mcf_update_rhs: new supplies / capacities under a resident basis
// Flows and states of non-basic arcs do not depend on supplies; tree flows are subtree sums of node balances, and a
// subtree is a contiguous range of the preorder.  Bytes each pass moves (n nodes, m arcs, k changes):
//   k_rhs_scatter  one lane per change: 12 B in; a capacity change reads and writes the arc's 16 B walk record (+ 1 B state,
//                  and 8 B reduced cost -> 4 B key code when a non-basic arc at capacity falls back to its lower bound);
//                  a supply change is one 8 B store.
//   k_rhs_balance  one lane per node: supply (8 B), position (4 B dense; 4 + 8 B blocked: slot, block base), and per
//                  adjacency entry (2 m of them) 8 B entry + 1 B state + 16 B walk record of the NON-BASIC arcs only;
//                  16 B out (the 128-bit balance, at the node's preorder position).
//   k_rhs_scan_*   inclusive prefix sum over the n + 1 positions in three launches (chunk totals, scan of the totals by one
//                  workgroup, scan of every chunk): 16 B per position read twice and written once.
//   k_rhs_flows    one lane per node: node record (16 B), position, two 16 B prefix sums, the tree arc's walk record read
//                  and its flow written (16 + 8 B); an artificial arc that turns round rewrites 4 B of the node record and
//                  seeds 16 B of a jump record.  Census by wave reduction, one atomic per wave and counter.
// All sums are 128-bit: 2^30 arcs at capacities below 2^60 stay below 2^91, so no prefix can wrap.
constexpr int kRhsThreads = kPassThreads;
constexpr int kRhsPer = 8;                             // positions per lane in the scan
constexpr int kRhsChunk = kRhsThreads * kRhsPer;       // positions per workgroup
enum { RHS_VIOL = 0, RHS_WRONG = 1, RHS_FLIPS = 2, RHS_MOVED = 3, RHS_HUGE = 4, RHS_COUNTERS = 5 };

__device__ __forceinline__ void rhs_count(unsigned long long* info, int which, int32_t mine) {
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&info[which], (unsigned long long)mine);
}

__global__ __launch_bounds__(kRhsThreads) void k_rhs_scatter(McfView v, int64_t n_sup, const int32_t* __restrict__ snode, const int64_t* __restrict__ sval,
                                                             int64_t* __restrict__ supply, int64_t n_cap, const int32_t* __restrict__ carc,
                                                             const int64_t* __restrict__ cval, unsigned long long* __restrict__ info) {
    const int64_t total = n_sup > n_cap ? n_sup : n_cap;
    const int64_t stride = (int64_t)gridDim.x * kRhsThreads;
    int32_t moved = 0;
    for (int64_t i = (int64_t)blockIdx.x * kRhsThreads + threadIdx.x; i < total; i += stride) {
        if (i < n_sup) supply[snode[i]] = sval[i];
        if (i >= n_cap) continue;
        const int32_t e = carc[i];
        const int64_t nc = cval[i];
        McfArcW w = v.arcw[e];
        if (w.cap == nc) continue;
        w.cap = nc;
        if (v.state[e] == -1) {   // non-basic at capacity: the flow follows the capacity
            ++moved;
            if (nc >= MCF_INF || nc == 0) {   // no capacity to sit at: back to the lower bound (mcf_apply_basis' state rule)
                v.state[e] = 1;
                w.flow = 0;
                if (v.vkey) v.vkey[e] = mcf_vkey(-v.rcache[e], v.vk_bigm, v.vk_half);
            } else {
                w.flow = nc;
            }
        }
        v.arcw[e] = w;
    }
    rhs_count(info, RHS_MOVED, moved);
}

__global__ __launch_bounds__(kRhsThreads) void k_rhs_balance(McfView v, int32_t cur, const int64_t* __restrict__ supply, const int64_t* __restrict__ adj_off,
                                                             const int64_t* __restrict__ adj, mcf_u128* __restrict__ bal) {
    const int32_t n = v.n_nodes - 1;
    for (int32_t u = blockIdx.x * kRhsThreads + threadIdx.x; u < n; u += gridDim.x * kRhsThreads) {
        int32_t slot = 0;
        const int32_t p = tree_pos(v, cur, u, &slot);
        if (p < 0) continue;   // (a broken record: the flow pass counts it as a violation)
        __int128 b = supply[u];
        const int64_t lo = adj_off[u], hi = adj_off[u + 1];
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t w = adj[k];
            const int64_t e = (w & 0xffffffff) >> 1;
            if (v.state[e] == 0) continue;   // basic arcs get their flow from the subtree sums
            const int64_t f = v.arcw[e].flow;
            b += (w & 1) ? -(__int128)f : (__int128)f;
        }
        bal[p] = (mcf_u128)b;
    }
}

// thread t of a workgroup owns positions [chunk base + t * kRhsPer, + kRhsPer): 128 contiguous bytes, 16-byte accesses
__global__ __launch_bounds__(kRhsThreads) void k_rhs_scan_totals(const mcf_u128* __restrict__ bal, int32_t count, mcf_u128* __restrict__ part) {
    __shared__ mcf_u128 s[kRhsThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kRhsChunk + (int64_t)threadIdx.x * kRhsPer;
    mcf_u128 sum = 0;
#pragma unroll
    for (int k = 0; k < kRhsPer; ++k) if (base + k < count) sum += bal[base + k];
    sum = wave_block_sum(sum, s);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// bal[p] <- sum of bal[0 .. p] (inclusive, in place)
__global__ __launch_bounds__(kRhsThreads) void k_rhs_scan_apply(mcf_u128* __restrict__ bal, int32_t count, const mcf_u128* __restrict__ part) {
    __shared__ mcf_u128 s[kRhsThreads];
    const int64_t base = (int64_t)blockIdx.x * kRhsChunk + (int64_t)threadIdx.x * kRhsPer;
    mcf_u128 x[kRhsPer];
    mcf_u128 sum = 0;
#pragma unroll
    for (int k = 0; k < kRhsPer; ++k) { x[k] = base + k < count ? bal[base + k] : (mcf_u128)0; sum += x[k]; x[k] = sum; }
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kRhsThreads; off <<= 1) {   // Hillis-Steele over the lanes' totals
        const mcf_u128 add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : (mcf_u128)0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const mcf_u128 before = part[blockIdx.x] + (threadIdx.x > 0 ? s[threadIdx.x - 1] : (mcf_u128)0);
#pragma unroll
    for (int k = 0; k < kRhsPer; ++k) if (base + k < count) bal[base + k] = x[k] + before;
}

// `keep`: a real tree arc's flow is stored even where it violates a bound, as long as its magnitude stays below 2^60 (the dual
// phase of mcf_update_rhs_dual pivots on these flows; RHS_HUGE counts the ones that do not fit)
__global__ __launch_bounds__(kRhsThreads) void k_rhs_flows(McfView v, int32_t cur, const mcf_u128* __restrict__ pre, int64_t bigm, McfJump* __restrict__ jump,
                                                           unsigned long long* __restrict__ info, int32_t keep) {
    const int32_t N = v.n_nodes, n = N - 1;
    const int64_t m = v.m;
    int32_t viol = 0, wrong = 0, flips = 0, huge = 0;
    for (int32_t u = blockIdx.x * kRhsThreads + threadIdx.x; u < n; u += gridDim.x * kRhsThreads) {
        const McfNode nd = v.node[u];
        int32_t slot = 0;
        const int32_t p = tree_pos(v, cur, u, &slot);
        if (p < 1 || nd.size < 1 || (int64_t)p + nd.size > N || nd.pred < 0) { ++viol; continue; }
        const __int128 x = (__int128)(pre[p + nd.size - 1] - pre[p - 1]);   // surplus the subtree of u sends up
        const int64_t a = nd.pred >> 1;
        const bool up = (nd.pred & 1) != 0;
        if (a < m) {
            const __int128 f = up ? x : -x;
            const int64_t cap = v.arcw[a].cap;
            if (f < 0 || f > cap || f >= MCF_INF) {
                ++viol;
                if (keep) { if (f > -(__int128)MCF_INF && f < (__int128)MCF_INF) v.arcw[a].flow = (int64_t)f; else ++huge; }
                continue;
            }
            v.arcw[a].flow = (int64_t)f;
            if ((up && cap < MCF_INF && f == cap) || (!up && f == 0)) ++wrong;
        } else {
            const __int128 ax = x < 0 ? -x : x;
            if (ax >= MCF_INF) { ++viol; ++huge; continue; }
            v.arcw[a].flow = (int64_t)ax;
            const bool nup = x >= 0;
            if (nup != up) {   // the arc turns round: pi[u] = pi[root] -+ big-M, and with it every potential below
                ++flips;
                v.node[u].pred = (int32_t)((a << 1) | (nup ? 1 : 0));
                jump[u].val = nup ? -2 * bigm : 2 * bigm;
            }
        }
    }
    rhs_count(info, RHS_VIOL, viol);
    rhs_count(info, RHS_WRONG, wrong);
    rhs_count(info, RHS_FLIPS, flips);
    if (keep) rhs_count(info, RHS_HUGE, huge);
}

// ------------------------------------------------------------------ mcf_add_arcs: merge new arcs into a resident handle
// A new arc enters non-basic at its lower bound with flow 0: flows, potentials, the tree and every existing reduced cost stay.
// What moves is the layout -- engine order is a total order (head bucket, tail, caller's index) and the k new arcs belong
// inside it.  Index arithmetic: mcf_core.h (mcf_topo_*).  All passes are out of place; the host swaps the pointers afterwards.
//   k_aa_new      one lane per new arc (sorted by key): its engine index (an upper bound on tail inside its bucket) and its
//                 static fields -- state +1, flow 0;
//   k_aa_scatter  ONE streaming pass over the old arcs in chunks of kAaChunk: old arcs are sorted by the same key, so their
//                 offset is monotone, and a chunk with the same offset at both ends is a shifted copy -- 16-byte loads, 16-byte
//                 stores where the offset keeps the alignment, no search per arc.  Other chunks search per arc.  Either way
//                 the map old index -> new index is left in emap[] for the adjacency and the node records;
//   k_aa_adj*     the adjacency: offsets, old entries (engine index remapped through emap), the 2k new entries appended to
//                 their nodes' lists;
//   k_aa_nodes    pred words: real arcs through emap, artificial ones + k;
//   k_aa_price    one lane per new arc: rc = cost + pi[tail] - pi[head], key code, census of the eligible ones.
constexpr int kAaThreads = 256;
constexpr int kAaChunk = kAaThreads * 4;

typedef int aa_int4 __attribute__((ext_vector_type(4)));
typedef long long aa_long2 __attribute__((ext_vector_type(2)));
template <bool NT, typename T>
__device__ __forceinline__ T aa_ld(const T* p) { return NT ? __builtin_nontemporal_load(p) : *p; }

struct AaArgs {
    int64_t m, k, per;                         // old arcs, new arcs, nodes per head bucket
    int64_t bucket_off[MCF_NUM_BUCKETS + 1];   // of the OLD layout
    // the new arcs, sorted by (bucket, tail, given order)
    const int64_t* nkey;                       // [k]
    const int32_t *ntail, *nhead, *ncost, *norig;
    const int64_t* ncap;
    const int8_t* nprio;                       // nullptr unless the handle keeps priorities
    int64_t* npos;                             // [k] out: engine index of every new arc
    // old arrays / new arrays (prio, rcache, vkey: nullptr where the handle has none)
    const int32_t *tail, *head, *cost, *orig;
    const int8_t *state, *prio;
    const int64_t* rcache;
    const int32_t* vkey;
    const McfArcW* arcw;
    int32_t *tail2, *head2, *cost2, *orig2;
    int8_t *state2, *prio2;
    int64_t* rcache2;
    int32_t* vkey2;
    McfArcW* arcw2;
    int32_t* emap;                             // [m] out: old engine index -> new engine index
    unsigned long long* info;                  // [0] arcs of shifted chunks, [1] eligible new arcs
};

__global__ __launch_bounds__(kAaThreads) void k_aa_new(AaArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kAaThreads;
    for (int64_t r = (int64_t)blockIdx.x * kAaThreads + threadIdx.x; r < a.k; r += stride) {
        const int64_t d = mcf_topo_new_index(r, a.nkey[r], a.tail, a.bucket_off);
        a.npos[r] = d;
        a.tail2[d] = a.ntail[r]; a.head2[d] = a.nhead[r]; a.cost2[d] = a.ncost[r]; a.orig2[d] = a.norig[r];
        a.state2[d] = 1;
        if (a.prio2) a.prio2[d] = a.nprio ? (int8_t)(a.nprio[r] & 3) : (int8_t)0;
        if (a.rcache2) a.rcache2[d] = 0;   // (k_aa_price fills both where the handle keeps them)
        if (a.vkey2) a.vkey2[d] = 0;
        McfArcW w;
        w.cap = a.ncap[r]; w.flow = 0;
        a.arcw2[d] = w;
    }
}

__device__ __forceinline__ void aa_move_one(const AaArgs& a, int64_t e, int64_t d) {
    a.tail2[d] = a.tail[e]; a.head2[d] = a.head[e]; a.cost2[d] = a.cost[e]; a.orig2[d] = a.orig[e];
    a.state2[d] = a.state[e];
    if (a.prio2) a.prio2[d] = a.prio[e];
    if (a.rcache2) a.rcache2[d] = a.rcache[e];
    if (a.vkey2) a.vkey2[d] = a.vkey[e];
    a.arcw2[d] = a.arcw[e];
    a.emap[e] = (int32_t)d;
}

template <bool NT>
__global__ __launch_bounds__(kAaThreads) void k_aa_scatter(AaArgs a) {
    const int64_t chunks = (a.m + kAaChunk - 1) / kAaChunk;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t lo = c * kAaChunk, hi = lo + kAaChunk < a.m ? lo + kAaChunk : a.m;
        // the offsets of the chunk's first and last arc (the same addresses in every lane: scalar loads)
        const int64_t off = mcf_count_below(a.nkey, a.k, mcf_topo_key(a.tail[lo], a.head[lo], a.per));
        const int64_t off_hi = mcf_count_below(a.nkey, a.k, mcf_topo_key(a.tail[hi - 1], a.head[hi - 1], a.per));
        if (off == off_hi) {
            // shifted copy: lane t owns arcs [e, e + 4), e a multiple of 4 (every array is padded to a multiple of 1024 arcs,
            // so the wide loads stay inside it; stores are cut at hi)
            const int64_t e = lo + 4 * (int64_t)threadIdx.x, d = e + off;
            if (threadIdx.x == 0) atomicAdd(&a.info[0], (unsigned long long)(hi - lo));
            if (e >= hi) continue;
            const aa_int4 t4 = aa_ld<NT>(reinterpret_cast<const aa_int4*>(a.tail + e)), h4 = aa_ld<NT>(reinterpret_cast<const aa_int4*>(a.head + e));
            const aa_int4 c4 = aa_ld<NT>(reinterpret_cast<const aa_int4*>(a.cost + e)), o4 = aa_ld<NT>(reinterpret_cast<const aa_int4*>(a.orig + e));
            const int32_t s4 = aa_ld<NT>(reinterpret_cast<const int32_t*>(a.state + e));
            const int32_t p4 = a.prio2 ? aa_ld<NT>(reinterpret_cast<const int32_t*>(a.prio + e)) : 0;
            aa_long2 r01 = {0, 0}, r23 = {0, 0};
            if (a.rcache2) { r01 = aa_ld<NT>(reinterpret_cast<const aa_long2*>(a.rcache + e)); r23 = aa_ld<NT>(reinterpret_cast<const aa_long2*>(a.rcache + e + 2)); }
            aa_int4 k4 = {0, 0, 0, 0};
            if (a.vkey2) k4 = aa_ld<NT>(reinterpret_cast<const aa_int4*>(a.vkey + e));
            aa_long2 w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = e + j < hi ? aa_ld<NT>(reinterpret_cast<const aa_long2*>(a.arcw + e + j)) : aa_long2{0, 0};
            const aa_int4 m4 = {(int32_t)d, (int32_t)d + 1, (int32_t)d + 2, (int32_t)d + 3};
            if (e + 4 <= hi) *reinterpret_cast<aa_int4*>(a.emap + e) = m4;
            else for (int j = 0; e + j < hi; ++j) a.emap[e + j] = m4[j];
            if ((off & 3) == 0 && e + 4 <= hi) {
                *reinterpret_cast<aa_int4*>(a.tail2 + d) = t4; *reinterpret_cast<aa_int4*>(a.head2 + d) = h4;
                *reinterpret_cast<aa_int4*>(a.cost2 + d) = c4; *reinterpret_cast<aa_int4*>(a.orig2 + d) = o4;
                *reinterpret_cast<int32_t*>(a.state2 + d) = s4;
                if (a.prio2) *reinterpret_cast<int32_t*>(a.prio2 + d) = p4;
                if (a.rcache2) { *reinterpret_cast<aa_long2*>(a.rcache2 + d) = r01; *reinterpret_cast<aa_long2*>(a.rcache2 + d + 2) = r23; }
                if (a.vkey2) *reinterpret_cast<aa_int4*>(a.vkey2 + d) = k4;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (e + j >= hi) break;
                    a.tail2[d + j] = t4[j]; a.head2[d + j] = h4[j]; a.cost2[d + j] = c4[j]; a.orig2[d + j] = o4[j];
                    a.state2[d + j] = (int8_t)(s4 >> (8 * j));
                    if (a.prio2) a.prio2[d + j] = (int8_t)(p4 >> (8 * j));
                    if (a.rcache2) a.rcache2[d + j] = j < 2 ? r01[j] : r23[j - 2];
                    if (a.vkey2) a.vkey2[d + j] = k4[j];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) if (e + j < hi) *reinterpret_cast<aa_long2*>(a.arcw2 + d + j) = w[j];
        } else {
            for (int64_t e = lo + threadIdx.x; e < hi; e += kAaThreads)
                aa_move_one(a, e, mcf_topo_old_index(e, mcf_topo_key(a.tail[e], a.head[e], a.per), a.nkey, a.k));
        }
    }
}

// adjacency offsets: one lane per node (n + 1 entries)
__global__ __launch_bounds__(kAaThreads) void k_aa_adj_off(const int64_t* __restrict__ off, int64_t count, const int64_t* __restrict__ ep_node, int64_t k2,
                                                           int64_t* __restrict__ off2) {
    const int64_t stride = (int64_t)gridDim.x * kAaThreads;
    for (int64_t u = (int64_t)blockIdx.x * kAaThreads + threadIdx.x; u < count; u += stride) off2[u] = mcf_topo_adj_off(off[u], u, ep_node, k2);
}
// old entries: one lane per entry
__global__ __launch_bounds__(kAaThreads) void k_aa_adj(const int64_t* __restrict__ adj, int64_t count, const int64_t* __restrict__ ep_end, int64_t k2,
                                                       const int32_t* __restrict__ emap, int64_t* __restrict__ adj2) {
    const int64_t stride = (int64_t)gridDim.x * kAaThreads;
    for (int64_t p = (int64_t)blockIdx.x * kAaThreads + threadIdx.x; p < count; p += stride) {
        const int64_t x = adj[p];
        const int64_t e = (x & 0xffffffffll) >> 1;
        adj2[mcf_topo_adj_index(p, ep_end, k2)] = (x & ~0xfffffffell) | ((int64_t)emap[e] << 1);
    }
}
// new entries: ep_val[j] = (other end point << 32) | (sorted rank of the arc << 1) | (1 when the node is the arc's tail)
__global__ __launch_bounds__(kAaThreads) void k_aa_adj_new(const int64_t* __restrict__ ep_val, const int64_t* __restrict__ ep_end, int64_t k2,
                                                           const int64_t* __restrict__ npos, int64_t* __restrict__ adj2) {
    const int64_t stride = (int64_t)gridDim.x * kAaThreads;
    for (int64_t j = (int64_t)blockIdx.x * kAaThreads + threadIdx.x; j < k2; j += stride) {
        const int64_t x = ep_val[j];
        adj2[ep_end[j] + j] = (x & ~0xfffffffell) | (npos[(x & 0xffffffffll) >> 1] << 1);
    }
}

__global__ __launch_bounds__(kAaThreads) void k_aa_nodes(const McfNode* __restrict__ node, int32_t n_nodes, int64_t m, int64_t k,
                                                         const int32_t* __restrict__ emap, McfNode* __restrict__ node2) {
    const int32_t stride = (int32_t)(gridDim.x * kAaThreads);
    for (int32_t v = (int32_t)(blockIdx.x * kAaThreads + threadIdx.x); v < n_nodes; v += stride) {
        McfNode r = node[v];
        if (r.pred >= 0) {
            const int64_t arc = r.pred >> 1;
            const int64_t arc2 = arc >= m ? arc + k : (int64_t)emap[arc];
            r.pred = (int32_t)((arc2 << 1) | (r.pred & 1));
        }
        node2[v] = r;
    }
}

// reduced costs / key codes of the new arcs (state +1: the violation is -rc) on the NEW arrays, and the census
__global__ __launch_bounds__(kAaThreads) void k_aa_price(McfView v, const int64_t* __restrict__ npos, int64_t k, int64_t* __restrict__ rcache,
                                                         int32_t* __restrict__ vkey, unsigned long long* __restrict__ info) {
    __shared__ int32_t s[kPassWaves];
    int32_t eligible = 0;
    const int64_t stride = (int64_t)gridDim.x * kAaThreads;
    for (int64_t r = (int64_t)blockIdx.x * kAaThreads + threadIdx.x; r < k; r += stride) {
        const int64_t e = npos[r];
        const int64_t rc = (int64_t)v.cost[e] + v.pi[v.tail[e]] - v.pi[v.head[e]];
        if (rcache) rcache[e] = rc;
        if (vkey) vkey[e] = mcf_vkey(-rc, v.vk_bigm, v.vk_half);
        eligible += rc < 0 ? 1 : 0;
    }
    const int32_t total = wave_block_sum(eligible, s);
    if (threadIdx.x == 0 && total > 0) atomicAdd(&info[1], (unsigned long long)total);
}

// ------------------------------------------------------------------ mcf_cost_ranges: cost ranging on the resident basis
// Logic: mcf_core.h (mcf_rng_*).  Everything is indexed by node, nothing by preorder position: the dense array and the
// blocked list need no separate code.  Bytes each pass moves (N = n + 1 nodes, m arcs, K levels, 20 B per node and level):
//   k_rng_depth  one lane per node record (16 B): the greatest depth, reduced by block_reduce / k_final; the host reads that
//                one word and sizes the tables with it;
//   k_rng_anc    one launch per level: anc[k][v] = anc[k-1][anc[k-1][v]] (4 B read + 4 B gathered, 4 B written; level 0 reads
//                the node record instead), and the level's two table rows set to "no arc" (16 B written);
//   k_rng_arcs   one lane per engine arc, workgroup b on head bucket b % 8 like k_cert_arcs: state (1 B); for a non-basic arc
//                tail, head, cost, orig (4 B each), two gathered potentials (8 B each), two gathered node records for the depths,
//                its own pair written at the caller's index (16 B), and per jump one gathered ancestor (4 B), one table cell
//                read (8 B) and an atomic min where the cell is still higher.  At most 3 K + 2 jumps per arc.  The pass is bound
//                by its gathers, not by its streams: no non-temporal variant;
//   k_rng_push   one launch per level K - 1 .. 1: one lane per node, both tables: 16 B read, 4 B ancestor, up to four cells
//                read and lowered;
//   k_rng_out    one lane per node: node record, level-0 cells (16 B), the tree arc's caller's index (4 B), 16 B written;
//   k_rng_gather one lane per requested index: 8 B index, 16 B gathered, 16 B written.
// Census by wave reduction, one atomic per wave and counter (rhs_count).
constexpr int kRngThreads = kPassThreads;
constexpr int kRngMaxBlocks = kCertMaxBlocks;                 // k_rng_arcs: at most 2 048 workgroups of 256 lanes, grid-stride beyond
enum { RNG_ELIGIBLE = 0, RNG_BASIC_REAL = 1, RNG_BASIC_ART = 2, RNG_INF_DOWN = 3, RNG_INF_UP = 4, RNG_COUNTERS = 5 };

struct RngArgs {
    int32_t K;                // levels
    int32_t count_inf;        // 1: the whole arrays are the answer, MCF_RNG_INF entries are counted as they are written
    int32_t* anc;             // [K][n_nodes]
    int64_t* tab[2];          // [K][n_nodes] each: 0 = P, 1 = N
    int64_t *down, *up;       // [m] caller's order
    unsigned long long* info; // [RNG_COUNTERS]
};

__global__ __launch_bounds__(kRngThreads) void k_rng_depth(const McfNode* __restrict__ node, int32_t n_nodes, McfRngDepthAcc* __restrict__ part) {
    __shared__ McfRngDepthAcc s_wave[kPassWaves];
    McfRngDepthAcc acc;
    mcf_acc_init(&acc);
    for (int32_t v = blockIdx.x * kRngThreads + threadIdx.x; v < n_nodes; v += gridDim.x * kRngThreads) {
        const int64_t d = node[v].depth;
        if (d > acc.depth) acc.depth = d;
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kRngThreads) void k_rng_anc(const McfNode* __restrict__ node, int32_t n_nodes, int32_t k, RngArgs a) {
    const int32_t root = n_nodes - 1;
    const size_t row = (size_t)k * n_nodes;
    const int32_t* __restrict__ below = k > 0 ? a.anc + row - n_nodes : nullptr;
    for (int32_t v = blockIdx.x * kRngThreads + threadIdx.x; v < n_nodes; v += gridDim.x * kRngThreads) {
        int32_t up;
        if (k == 0) {
            const int32_t p = node[v].parent;
            up = (v == root || p < 0 || p >= n_nodes) ? root : p;
        } else {
            up = below[below[v]];
        }
        a.anc[row + v] = up;
        a.tab[0][row + v] = MCF_RNG_INF;
        a.tab[1][row + v] = MCF_RNG_INF;
    }
}

__global__ __launch_bounds__(kRngThreads) void k_rng_arcs(McfView v, RngArgs a) {
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
    const int32_t N = v.n_nodes;
    int32_t eligible = 0, inf_down = 0, inf_up = 0;
    for (int64_t e = lo + lb * kRngThreads + threadIdx.x; e < hi; e += nlb * kRngThreads) {
        const int32_t st = v.state[e];
        if (st == 0) continue;   // basic arcs get their pair from the tables (k_rng_out); padding has none
        const int32_t t = v.tail[e], hd = v.head[e];
        const int64_t s = mcf_rng_slack(st, (int64_t)v.cost[e] + v.pi[t] - v.pi[hd]);
        if (s < 0) ++eligible;
        const int64_t o = v.orig[e];
        int64_t dn, up;
        mcf_rng_nonbasic(st, s, &dn, &up);
        a.down[o] = dn; a.up[o] = up;
        if (dn == MCF_RNG_INF) ++inf_down;
        if (up == MCF_RNG_INF) ++inf_up;
        mcf_rng_jumps(t, v.node[t].depth, hd, v.node[hd].depth, a.K,
                      [&](int k, int32_t y) { return a.anc[(size_t)k * N + y]; },
                      [&](int side, int k, int32_t y) { mcf_rng_lower(a.tab[mcf_rng_table(st, side == 0)] + (size_t)k * N + y, s); });
    }
    rhs_count(a.info, RNG_ELIGIBLE, eligible);
    if (a.count_inf) { rhs_count(a.info, RNG_INF_DOWN, inf_down); rhs_count(a.info, RNG_INF_UP, inf_up); }
}

__global__ __launch_bounds__(kRngThreads) void k_rng_push(int32_t n_nodes, int32_t k, RngArgs a) {
    const size_t row = (size_t)k * n_nodes, low = row - n_nodes;
    for (int32_t y = blockIdx.x * kRngThreads + threadIdx.x; y < n_nodes; y += gridDim.x * kRngThreads) {
        const int64_t p = a.tab[0][row + y], q = a.tab[1][row + y];
        if (p == MCF_RNG_INF && q == MCF_RNG_INF) continue;
        const int32_t up = a.anc[low + y];
        mcf_rng_push(p, a.tab[0] + low + y, a.tab[0] + low + up);
        mcf_rng_push(q, a.tab[1] + low + y, a.tab[1] + low + up);
    }
}

__global__ __launch_bounds__(kRngThreads) void k_rng_out(McfView v, RngArgs a) {
    const int32_t n = v.n_nodes - 1;
    const int64_t m = v.m;
    int32_t real = 0, art = 0, inf_down = 0, inf_up = 0;
    for (int32_t u = blockIdx.x * kRngThreads + threadIdx.x; u < n; u += gridDim.x * kRngThreads) {
        const int32_t pred = v.node[u].pred;
        if (pred < 0) continue;
        const int64_t arc = pred >> 1;
        if (arc >= m) { ++art; continue; }   // an artificial tree arc has no caller's cost: the minima recorded on it are never read out
        ++real;
        int64_t dn, up;
        mcf_rng_basic((pred & 1) != 0, a.tab[0][u], a.tab[1][u], &dn, &up);
        const int64_t o = v.orig[arc];
        a.down[o] = dn; a.up[o] = up;
        if (dn == MCF_RNG_INF) ++inf_down;
        if (up == MCF_RNG_INF) ++inf_up;
    }
    rhs_count(a.info, RNG_BASIC_REAL, real);
    rhs_count(a.info, RNG_BASIC_ART, art);
    if (a.count_inf) { rhs_count(a.info, RNG_INF_DOWN, inf_down); rhs_count(a.info, RNG_INF_UP, inf_up); }
}

__global__ __launch_bounds__(kRngThreads) void k_rng_gather(int64_t count, const int64_t* __restrict__ idx, const int64_t* __restrict__ down,
                                                            const int64_t* __restrict__ up, int64_t* __restrict__ gdown, int64_t* __restrict__ gup,
                                                            unsigned long long* __restrict__ info) {
    int32_t inf_down = 0, inf_up = 0;
    for (int64_t i = (int64_t)blockIdx.x * kRngThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kRngThreads) {
        const int64_t o = idx[i];
        const int64_t dn = down[o], u = up[o];
        gdown[i] = dn; gup[i] = u;
        if (dn == MCF_RNG_INF) ++inf_down;
        if (u == MCF_RNG_INF) ++inf_up;
    }
    rhs_count(info, RNG_INF_DOWN, inf_down);
    rhs_count(info, RNG_INF_UP, inf_up);
}

// ------------------------------------------------------------------ mcf_supply_ranges / mcf_capacity_ranges: flow ranging on the resident basis
// Logic: mcf_core.h (mcf_frng_*).  Indexed by node like k_rng_*: both tree layouts run the same code.  The ancestors
// (anc[k][v]) and the two 8-byte tables are the arrays of cost ranging, here U and D; two 4-byte tables beside them hold the
// attaining node.  Gather only: no cell is written by more than one lane, there is no atomic but the census.  Bytes each pass
// moves (N = n + 1 nodes, m arcs, K levels, 28 B per node and level):
//   k_rng_depth   as for cost ranging: the greatest depth, one word back to the host;
//   k_frng_base   one lane per node: node record (16 B), the tree arc's walk record gathered (16 B), level 0 written (28 B);
//   k_frng_level  one launch per level 1 .. K - 1: the lane's own cells of the level below (28 B), the cells of its ancestor
//                 there gathered (28 B), one level written (28 B);
//   k_frng_pairs  one lane per pair: two node ids (8 B), two gathered node records for the depths, two potentials (8 B each);
//                 per jump one gathered ancestor (4 B) and one gathered cell (12 B), a node record for a level-0 jump;
//                 at most 3 K + 2 jumps; the attaining node's record and its arc's caller's index (16 + 4 B); 28 B written;
//   k_frng_arcs   one lane per engine arc, workgroup b on head bucket b % 8 like k_rng_arcs: state (1 B), walk record (16 B),
//                 orig (4 B), 40 B written at the caller's index; an arc at capacity besides tail, head, cost (4 B each), two
//                 potentials, two node records, and per jump one ancestor and BOTH cells (24 B): its two pushes share one
//                 enumeration.  Bound by its gathers like k_rng_arcs: no non-temporal variant;
//   k_frng_gather one lane per requested index: 8 B index, 40 B gathered, 40 B written.
// Census by wave reduction, one atomic per wave and counter (rhs_count).
constexpr int kFrngThreads = kPassThreads;
constexpr int kFrngMaxBlocks = kRngMaxBlocks;
enum { FRNG_BASIC_REAL = 0, FRNG_BASIC_ART = 1, FRNG_AT_CAP = 2, FRNG_INF = 3, FRNG_ZERO = 4, FRNG_RISING = 5, FRNG_COUNTERS = 6 };

struct FrngArgs {
    int32_t K;                 // levels
    int32_t count_sides;       // k_frng_arcs: 1 = the whole arrays are the answer, INF and 0 sides are counted as they are written
    int32_t* anc;              // [K][n_nodes]
    int64_t* val[2];           // [K][n_nodes] each: 0 = U, 1 = D
    int32_t* id[2];            // [K][n_nodes] each: the attaining node
    int64_t* out;              // k_frng_arcs: [5][m] down, up, down_arc, up_arc, rate in the caller's order
    unsigned long long* info;  // [FRNG_COUNTERS]
};

// the attaining node as a caller's index: its tree arc through orig, m + v for an artificial one
__device__ __forceinline__ int64_t frng_index(const McfView& v, int32_t node) {
    if (node < 0) return -1;
    const int64_t a = v.node[node].pred >> 1;
    return a >= v.m ? a : (int64_t)v.orig[a];
}

__global__ __launch_bounds__(kFrngThreads) void k_frng_base(McfView v, FrngArgs a) {
    const int32_t N = v.n_nodes, root = N - 1;
    int32_t real = 0, art = 0;
    for (int32_t u = blockIdx.x * kFrngThreads + threadIdx.x; u < N; u += gridDim.x * kFrngThreads) {
        const McfNode nd = v.node[u];
        int64_t U = MCF_RNG_INF, D = MCF_RNG_INF;
        int32_t id = -1;
        if (u != root && nd.pred >= 0 && (int64_t)(nd.pred >> 1) < v.m + root) {   // (a record that names no arc limits nothing)
            const int64_t arc = nd.pred >> 1;
            const McfArcW w = v.arcw[arc];
            mcf_frng_residuals(nd.pred, v.m, w.cap, w.flow, &U, &D);
            id = u;
            if (arc >= v.m) ++art; else ++real;
        }
        a.anc[u] = mcf_rng_anc0(u, nd.parent, N);
        a.val[0][u] = U; a.val[1][u] = D;
        a.id[0][u] = id; a.id[1][u] = id;
    }
    rhs_count(a.info, FRNG_BASIC_REAL, real);
    rhs_count(a.info, FRNG_BASIC_ART, art);
}

__global__ __launch_bounds__(kFrngThreads) void k_frng_level(int32_t n_nodes, int32_t k, FrngArgs a) {
    const size_t row = (size_t)k * n_nodes, low = row - n_nodes;
    for (int32_t u = blockIdx.x * kFrngThreads + threadIdx.x; u < n_nodes; u += gridDim.x * kFrngThreads) {
        const int32_t up = a.anc[low + u];
        a.anc[row + u] = a.anc[low + up];
        const McfFrngMin U = mcf_frng_up({a.val[0][low + u], a.id[0][low + u]}, {a.val[0][low + up], a.id[0][low + up]});
        const McfFrngMin D = mcf_frng_down({a.val[1][low + u], a.id[1][low + u]}, {a.val[1][low + up], a.id[1][low + up]});
        a.val[0][row + u] = U.val; a.id[0][row + u] = U.id;
        a.val[1][row + u] = D.val; a.id[1][row + u] = D.id;
    }
}

__global__ __launch_bounds__(kFrngThreads) void k_frng_pairs(McfView v, FrngArgs a, int64_t count, const int32_t* __restrict__ from, const int32_t* __restrict__ to,
                                                             int64_t* __restrict__ limit, int64_t* __restrict__ limit_arc, int64_t* __restrict__ rate,
                                                             int32_t* __restrict__ rising) {
    const int32_t N = v.n_nodes;
    int32_t n_inf = 0, n_zero = 0, n_rising = 0;
    for (int64_t i = (int64_t)blockIdx.x * kFrngThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kFrngThreads) {
        const int32_t x = from[i], y = to[i];
        McfFrngPush p;
        mcf_frng_push(x, y, a.K, v.m,
                      [&](int k, int32_t u) { return a.anc[(size_t)k * N + u]; },
                      [&](int w, int k, int32_t u) { return McfFrngMin{a.val[w][(size_t)k * N + u], a.id[w][(size_t)k * N + u]}; },
                      [&](int32_t u) { return v.node[u].depth; }, [&](int32_t u) { return v.node[u].pred; }, &p);
        const McfFrngMin r = mcf_frng_end(p);
        limit[i] = r.val;
        limit_arc[i] = frng_index(v, r.id);
        rate[i] = v.pi[y] - v.pi[x];
        rising[i] = p.rising;
        if (r.val == MCF_RNG_INF) ++n_inf;
        if (r.val == 0) ++n_zero;
        if (p.rising > 0) ++n_rising;
    }
    rhs_count(a.info, FRNG_INF, n_inf);
    rhs_count(a.info, FRNG_ZERO, n_zero);
    rhs_count(a.info, FRNG_RISING, n_rising);
}

__global__ __launch_bounds__(kFrngThreads) void k_frng_arcs(McfView v, FrngArgs a) {
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
    const int32_t N = v.n_nodes;
    const int64_t m = v.m;
    int32_t at_cap = 0, n_inf = 0, n_zero = 0, n_rising = 0;
    for (int64_t e = lo + lb * kFrngThreads + threadIdx.x; e < hi; e += nlb * kFrngThreads) {
        const int32_t st = v.state[e];
        const McfArcW w = v.arcw[e];
        const int64_t o = v.orig[e];
        int64_t rc = 0;
        McfFrngMin fwd = {MCF_RNG_INF, -1}, back = {MCF_RNG_INF, -1};
        if (mcf_frng_needs_push(st, w.cap)) {
            ++at_cap;
            const int32_t t = v.tail[e], hd = v.head[e];
            rc = (int64_t)v.cost[e] + v.pi[t] - v.pi[hd];
            McfFrngPush pf, pb;
            mcf_frng_push_both(t, hd, a.K, m,
                               [&](int k, int32_t u) { return a.anc[(size_t)k * N + u]; },
                               [&](int w, int k, int32_t u) { return McfFrngMin{a.val[w][(size_t)k * N + u], a.id[w][(size_t)k * N + u]}; },
                               [&](int32_t u) { return v.node[u].depth; }, [&](int32_t u) { return v.node[u].pred; }, &pf, &pb);
            fwd = mcf_frng_end(pf);
            back = mcf_frng_end(pb);
            n_rising += (pf.rising > 0) + (pb.rising > 0);
        }
        const McfFrngArc r = mcf_frng_arc(st, w.cap, w.flow, rc, o, fwd.val, frng_index(v, fwd.id), back.val, frng_index(v, back.id));
        a.out[o] = r.down; a.out[m + o] = r.up; a.out[2 * m + o] = r.down_arc; a.out[3 * m + o] = r.up_arc; a.out[4 * m + o] = r.rate;
        n_inf += (r.down == MCF_RNG_INF) + (r.up == MCF_RNG_INF);
        n_zero += (r.down == 0) + (r.up == 0);
    }
    rhs_count(a.info, FRNG_AT_CAP, at_cap);
    rhs_count(a.info, FRNG_RISING, n_rising);
    if (a.count_sides) { rhs_count(a.info, FRNG_INF, n_inf); rhs_count(a.info, FRNG_ZERO, n_zero); }
}

// rows of `out` ([5][m]) at the indices asked -> `g` ([5][count])
__global__ __launch_bounds__(kFrngThreads) void k_frng_gather(int64_t count, int64_t m, const int64_t* __restrict__ idx, const int64_t* __restrict__ out,
                                                              int64_t* __restrict__ g, unsigned long long* __restrict__ info) {
    int32_t n_inf = 0, n_zero = 0;
    for (int64_t i = (int64_t)blockIdx.x * kFrngThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kFrngThreads) {
        const int64_t o = idx[i];
        const int64_t dn = out[o], up = out[m + o];
        g[i] = dn; g[count + i] = up; g[2 * count + i] = out[2 * m + o]; g[3 * count + i] = out[3 * m + o]; g[4 * count + i] = out[4 * m + o];
        n_inf += (dn == MCF_RNG_INF) + (up == MCF_RNG_INF);
        n_zero += (dn == 0) + (up == 0);
    }
    rhs_count(info, FRNG_INF, n_inf);
    rhs_count(info, FRNG_ZERO, n_zero);
}

// ------------------------------------------------------------------ mcf_update_rhs_dual: dual pivots on the resident arrays
// The rule is in include/mcf.h, the choices and the forced decide in mcf_core.h.  One dual pivot is five launches:
//   k_dual_leave   one lane per node: node record (16 B) and the tree arc's walk record (16 B); arg-max of the violations
//                  per workgroup (block_reduce), k_final<McfDualLeave> merges the partials.
//   k_dual_enter   every lane reads the winner (q, its record, position and flow: five scalar loads), then one of
//       sweep:     the streaming pass of k_cut_arcs -- tail, head (4 B each), state (1 B) of every arc, and for the
//                  non-basic ones two gathered positions (4 B dense; 4 + 8 B blocked); an arc across the cut adds its
//                  capacity (8 B), caller's index (4 B) and reduced cost (8 B resident, else cost + two potentials);
//       walk:      |S| <= enter_walk: the nodes at the positions of S (dense: order[]; blocked list: the slots of the blocks
//                  that meet the range) walk their adjacency lists: 8 B per entry, state, and for the non-basic arcs the
//                  other end's position and the same three words.  Every arc across the cut is met once, from inside.
//                  Both reduce to one McfDualEnter per workgroup; arg-min and tie rule do not depend on the order.
//   k_pivot_dual   one workgroup: merges the candidates, begins (the pending flip), finds the cycle with k_pivot's climb /
//                  scan, decides with the leaving arc given (mcf_pivot_decide_forced) and finishes (mcf_pivot_finish).
//   launch_apply   unchanged.
// After the last pivot k_dual_close sweeps the arcs once: a closed arc whose slack turned negative changes its state.
// Status and counters live in one DualState record; the host reads it once per batch of queued pivots.
enum { DUAL_RUNNING = 0, DUAL_CLEARED = 1, DUAL_NO_ENTERING = 2, DUAL_BUDGET = 3, DUAL_MAGNITUDE = 4, DUAL_INTERNAL = 5 };
struct DualState {
    int64_t status;       // DUAL_*
    int64_t pivots;       // dual pivots made
    int64_t max_pivots;   // the budget
    int64_t sweeps, walks;
};
struct DualArgs {
    const McfCtx* ctx;
    const McfDualLeave* leave;   // the merged arg-max
    const struct DualState* st;  // the phase's status record: once it has stopped, the launches still queued do nothing
    const int64_t* adj_off;      // full adjacency (the handle's, or the certificate's own)
    const int64_t* adj;
    int32_t walk_max;            // walk when |S| <= this (0: always sweep)
};

// the view of the tree a pass between two pivots sees: a flip the last update left pending counted (tree_sel on the host)
struct DualSel { int32_t cur, arena, nblk; };
__device__ __forceinline__ DualSel dual_sel(const McfCtx* c) {
    const int32_t pf = c->pending_flip ? 1 : 0;
    return DualSel{c->cur ^ pf, c->arena ^ ((pf && c->rebuild) ? 1 : 0), c->alloc_next};
}

__global__ __launch_bounds__(kPassThreads) void k_dual_leave(McfView v, const DualState* __restrict__ st, McfDualLeave* __restrict__ part) {
    __shared__ McfDualLeave s_wave[kPassWaves];
    const int32_t n = st->status == DUAL_RUNNING ? v.n_nodes - 1 : 0;   // (uniform; a stopped phase: empty partials)
    const int64_t narc = v.m + n;
    McfDualLeave acc;
    mcf_acc_init(&acc);
    for (int32_t u = blockIdx.x * kPassThreads + threadIdx.x; u < n; u += gridDim.x * kPassThreads) {
        const int32_t pred = v.node[u].pred;
        if (pred < 0 || (int64_t)(pred >> 1) >= narc) continue;
        const McfArcW w = v.arcw[pred >> 1];
        mcf_dual_leave_add(&acc, mcf_dual_violation(w.cap, w.flow), u, w.flow);
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// slack of a non-basic arc across the cut, into the lane's accumulator
template <bool NT>
__device__ __forceinline__ void dual_enter_arc(const McfView& v, McfDualEnter* acc, int64_t e, int32_t t, int32_t hd, int32_t st, bool tail_in, bool head_in,
                                               bool exports) {
    const int64_t cap = cert_ld<NT>(reinterpret_cast<const int64_t*>(v.arcw + e));
    if (!mcf_dual_candidate(st, cap, tail_in, head_in, exports)) return;
    const int64_t rc = (v.rcache && !v.rc_partial) ? cert_ld<NT>(v.rcache + e) : (int64_t)v.cost[e] + v.pi[t] - v.pi[hd];
    mcf_dual_enter_add(acc, (int64_t)st * rc, mcf_pack_arc(cert_ld<NT>(v.orig + e), e));
}

template <bool NT>
__global__ __launch_bounds__(kPassThreads) void k_dual_enter(McfView v, DualArgs a, McfDualEnter* __restrict__ part) {
    __shared__ McfDualEnter s_wave[kPassWaves];
    McfDualEnter acc;
    mcf_acc_init(&acc);
    const int32_t n = v.n_nodes - 1;
    const int64_t q = a.st->status == DUAL_RUNNING ? a.leave->node : (int64_t)-1;   // (a stopped phase: empty partials)
    if (q >= 0 && q < n) {   // (uniform)
        const DualSel sel = dual_sel(a.ctx);
        const McfNode rq = v.node[q];
        int32_t slot = 0;
        const int32_t pq = tree_pos(v, sel.cur, (int32_t)q, &slot), zq = rq.size;
        const int64_t qa = rq.pred >> 1;
        if (pq >= 1 && zq >= 1 && (int64_t)pq + zq <= v.n_nodes && rq.pred >= 0 && qa < v.m + n) {
            const bool exports = mcf_dual_exports((rq.pred & 1) != 0, v.arcw[qa].flow);
            if (zq > a.walk_max) {
                // ---- sweep: workgroup b on head bucket b % 8
                const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
                const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
                const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
                for (int64_t e = lo + lb * kPassThreads + threadIdx.x; e < hi; e += nlb * kPassThreads) {
                    const int32_t st = cert_ld<NT>(v.state + e);
                    if (st == 0) continue;
                    const int32_t t = cert_ld<NT>(v.tail + e), hd = cert_ld<NT>(v.head + e);
                    const bool tin = mcf_dual_in_subtree(tree_pos(v, sel.cur, t, &slot), pq, zq);
                    const bool hin = mcf_dual_in_subtree(tree_pos(v, sel.cur, hd, &slot), pq, zq);
                    if (tin != hin) dual_enter_arc<NT>(v, &acc, e, t, hd, st, tin, hin, exports);
                }
            } else {
                // ---- walk: one lane per node of S
                const int64_t gtid = (int64_t)blockIdx.x * kPassThreads + threadIdx.x, gsize = (int64_t)gridDim.x * kPassThreads;
                auto node_walk = [&](int32_t u) {
                    for (int64_t k = a.adj_off[u]; k < a.adj_off[u + 1]; ++k) {
                        const int64_t w = a.adj[k];
                        const int64_t e = (w & 0xffffffff) >> 1;
                        const int32_t other = (int32_t)(w >> 32);
                        const int32_t st = v.state[e];
                        if (st == 0 || other < 0 || other >= n) continue;
                        if (mcf_dual_in_subtree(tree_pos(v, sel.cur, other, &slot), pq, zq)) continue;
                        const bool is_tail = (w & 1) != 0;
                        dual_enter_arc<false>(v, &acc, e, is_tail ? u : other, is_tail ? other : u, st, is_tail, !is_tail, exports);
                    }
                };
                if (MCF_HAS_BPL(v)) {
                    const int32_t bs = v.blk_shift;
                    const McfBlkMeta* bm = sel.cur ? v.bmeta[1] : v.bmeta[0];
                    const int32_t* xa = sel.arena ? v.bext[1] : v.bext[0];
                    const int32_t* tok = sel.arena ? v.order[1] : v.order[0];
                    const int32_t* psz = sel.arena ? v.psz[1] : v.psz[0];
                    const int32_t nblk = sel.nblk < v.blk_cap ? sel.nblk : v.blk_cap;
                    for (int32_t b = blockIdx.x; b < nblk; b += gridDim.x) {   // (uniform per workgroup)
                        const McfBlkMeta mb = bm[b];
                        if (mb.base == MCF_BLK_FREE) continue;
                        const int32_t xe = xa[b];
                        int32_t o0 = mcf_ext_beg(xe), o1 = mcf_ext_end(xe);
                        if (pq - mb.base > o0) o0 = pq - mb.base;
                        if (pq + zq - mb.base < o1) o1 = pq + zq - mb.base;
                        for (int32_t o = o0 + (int32_t)threadIdx.x; o < o1; o += kPassThreads) {
                            const int32_t sl = (b << bs) + o;
                            if (psz[sl] == 0) continue;   // an empty slot
                            const int32_t u = tok[sl];
                            int32_t s2 = 0;
                            if (u < 0 || u >= n || tree_pos(v, sel.cur, u, &s2) != mb.base + o) continue;
                            node_walk(u);
                        }
                    }
                } else {
                    const int32_t* ord = sel.cur ? v.order[1] : v.order[0];
                    for (int64_t i = gtid; i < zq; i += gsize) {
                        const int32_t u = ord[pq + i];
                        if (u >= 0 && u < n) node_walk(u);
                    }
                }
            }
        }
    }
    block_reduce(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

template <bool BPL>
__global__ __launch_bounds__(kPivotThreads) void k_pivot_dual(McfView g, DualArgs a, const McfDualEnter* __restrict__ part, int npart, DualState* __restrict__ st,
                                                              int64_t* __restrict__ log, int64_t log_cap) {
    __shared__ PivotShared S;
    __shared__ int32_t s_q, s_qdepth, s_first_in, s_lstate;
    __shared__ int64_t s_delta;
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(&S.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(g.ctx)[threadIdx.x];
    // the candidates: least slack, ties to the lowest caller's index -- as an arg-max of (2^62 - slack) with k_pivot's reduction
    int64_t key = 0, arc = -1;
    for (int i = threadIdx.x; i < npart; i += kPivotThreads) {
        const McfDualEnter c = part[i];
        const int64_t kk = c.arc >= 0 ? ((int64_t)1 << 62) - c.slack : 0;
        if (c.arc >= 0 && mcf_cand_better(kk, c.arc, key, arc)) { key = kk; arc = c.arc; }
    }
    block_argmax<kPivotThreads>(key, arc);   // (its barrier also covers the control block)
    McfView v = g;
    v.ctx = &S.ctx;
    v.dirty = nullptr;   // every mark is raised again when the call ends (uc_finish)
    if (!BPL) { v.bmeta[0] = nullptr; v.bmeta[1] = nullptr; }
    const McfPaths gp = mcf_view_paths(v);
    const McfPaths sp = McfPaths{S.path[0], S.path[1], S.rec[0], S.rec[1], S.ppos[0], S.ppos[1], S.flow[0], S.flow[1], S.pslot[0], S.pslot[1]};
    const int32_t n = v.n_nodes - 1;
    if (threadIdx.x == 0) {
        McfCtx* c = v.ctx;
        int go = 0;
        int64_t stop = st->status;
        const McfDualLeave L = *a.leave;
        const int64_t q = L.node;
        if (stop == DUAL_RUNNING) {
            if (q < 0 || q >= n) stop = DUAL_CLEARED;
            else if (mcf_dual_too_large(L)) stop = DUAL_MAGNITUDE;
            else if (st->pivots >= st->max_pivots) stop = DUAL_BUDGET;
            else if (arc < 0 || key <= 0) stop = DUAL_NO_ENTERING;
        }
        mcf_pivot_begin_dual(v, stop == DUAL_RUNNING ? arc : (int64_t)-1, &S.cy);   // (the pending flip in every case)
        if (stop == DUAL_RUNNING) {
            const McfNode rq = v.node[q];
            const int64_t qflow = v.arcw[rq.pred >> 1].flow, qcap = v.arcw[rq.pred >> 1].cap;
            int32_t slot = 0;
            const int32_t pq = mcf_node_pos(v, c, (int32_t)q, &slot);
            const bool fin = mcf_dual_in_subtree(mcf_node_pos(v, c, c->pv_first, &slot), pq, rq.size);
            const bool sin = mcf_dual_in_subtree(mcf_node_pos(v, c, c->pv_second, &slot), pq, rq.size);
            const int64_t viol = mcf_dual_violation(qcap, qflow);
            if (fin == sin || viol != L.viol || c->pv_s == 0) stop = DUAL_INTERNAL;   // (the passes disagree: never pivot on that)
            else {
                s_q = (int32_t)q; s_qdepth = rq.depth; s_first_in = fin ? 1 : 0; s_lstate = mcf_dual_leave_state(qflow); s_delta = viol;
                const int32_t deep = S.cy.ru.depth > S.cy.rw.depth ? S.cy.ru.depth : S.cy.rw.depth;
                const bool gate = v.psz[0] && deep <= c->climb_depth && deep < kSmallPath;
                bool ok;
                if (gate) { ok = mcf_pivot_climb(v, sp, &S.cy, INT32_MAX); S.cy.small = 1; }
                else ok = mcf_pivot_climb(v, gp, &S.cy, mcf_climb_budget(v, S.cy));
                if (ok) go = S.cy.u == S.cy.w ? 1 : 2;
                else stop = DUAL_INTERNAL;
                if (go == 2) mcf_scan_init(&S.acc);
                // the log entry: leaving arc, entering arc (caller's indices), delta, slack
                if (ok && st->pivots < log_cap) {
                    const int64_t la = rq.pred >> 1, at = st->pivots * 4;
                    log[at] = la < v.m ? (int64_t)v.orig[la] : la;
                    log[at + 1] = arc >> 32;
                    log[at + 2] = viol;
                    log[at + 3] = ((int64_t)1 << 62) - key;
                }
            }
        }
        if (stop != DUAL_RUNNING) st->status = stop;
        S.go = go;
    }
    __syncthreads();
    const int go = S.go;
    if (go == 2) mcf_pivot_scan(v, sp, kSmallPath, &S.cy, &S.acc, S.hits, kHitsLds, threadIdx.x, kPivotThreads);  // barriers inside
    if (go && threadIdx.x == 0) {
        if (S.ctx.status == MCF_RUNNING && S.cy.u == S.cy.w) {
            const bool sm = S.cy.small != 0;
            const McfPaths pp = McfPaths{sm ? sp.path1 : gp.path1, sm ? sp.path2 : gp.path2, sm ? sp.rec1 : gp.rec1, sm ? sp.rec2 : gp.rec2,
                                         sm ? sp.ppos1 : gp.ppos1, sm ? sp.ppos2 : gp.ppos2, sm ? sp.flow1 : gp.flow1, sm ? sp.flow2 : gp.flow2,
                                         sm ? sp.slot1 : gp.slot1, sm ? sp.slot2 : gp.slot2};
            mcf_pivot_decide_forced(v, pp, S.cy, s_q, s_qdepth, s_first_in != 0, s_delta, s_lstate);
        }
        if (S.ctx.stage == 2) {
            const bool walked = S.ctx.t2_size <= a.walk_max;
            st->pivots += 1;
            if (walked) st->walks += 1; else st->sweeps += 1;
        } else {
            st->status = DUAL_INTERNAL;   // (status word of the control block says why, where it does)
        }
    }
    __syncthreads();
    if (go && S.cy.small) mcf_pivot_finish(v, sp, threadIdx.x, kPivotThreads);
    else mcf_pivot_finish(v, gp, threadIdx.x, kPivotThreads);
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(g.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(&S.ctx)[threadIdx.x];
}

// the end of the phase: closed arcs whose slack turned negative change their state (mcf_dual_closed_state); 1 B + 8 B per
// non-basic arc in, and the reduced cost of the closed ones
template <bool NT>
__global__ __launch_bounds__(kPassThreads) void k_dual_close(McfView v) {
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
    for (int64_t e = lo + lb * kPassThreads + threadIdx.x; e < hi; e += nlb * kPassThreads) {
        const int32_t st = cert_ld<NT>(v.state + e);
        if (st == 0 || cert_ld<NT>(reinterpret_cast<const int64_t*>(v.arcw + e)) != 0) continue;
        const int64_t rc = (v.rcache && !v.rc_partial) ? v.rcache[e] : (int64_t)v.cost[e] + v.pi[v.tail[e]] - v.pi[v.head[e]];
        const int32_t ns = mcf_dual_closed_state(st, 0, rc);
        if (ns == st) continue;
        v.state[e] = (int8_t)ns;
        if (v.vkey) v.vkey[e] = mcf_vkey(-(int64_t)ns * rc, v.vk_bigm, v.vk_half);
    }
}

// real non-basic arcs with a negative slack: more than none and the basis is not dual feasible
template <bool NT>
__global__ __launch_bounds__(kPassThreads) void k_dual_census(McfView v, unsigned long long* __restrict__ count) {
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
    int32_t bad = 0;
    for (int64_t e = lo + lb * kPassThreads + threadIdx.x; e < hi; e += nlb * kPassThreads) {
        const int32_t st = cert_ld<NT>(v.state + e);
        if (st == 0) continue;
        const int64_t rc = (v.rcache && !v.rc_partial) ? cert_ld<NT>(v.rcache + e)
                                                        : (int64_t)cert_ld<NT>(v.cost + e) + v.pi[cert_ld<NT>(v.tail + e)] - v.pi[cert_ld<NT>(v.head + e)];
        if ((int64_t)st * rc < 0) ++bad;
    }
    rhs_count(count, 0, bad);
}
