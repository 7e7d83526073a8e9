// mcf_engine.hip -- MI355X (gfx950) network-simplex pivot engine: HIP kernels + C ABI.
//
// One pivot, by instance size (mcf_create picks; all paths share mcf_core.h and give the same pivot sequence):
//
//   k_solve_small   whole instance in LDS: one persistent workgroup -- 256 lanes (one wave per SIMD), 1 024 when
//                   MCF_SMALL_THREADS asks (small_threads_for) -- prices (Dantzig / candidate list: the arcs' invariant
//                   data in registers, 10 or 3 arcs per lane by width; Devex: from LDS), pivots (the lanes stride over the
//                   tree nodes in the cycle search; every wave runs the ratio tests and takes the pivot's scalar decisions
//                   itself, the control block in its registers) and updates until the solve ends.  Dantzig with the plain key
//                   on an instance whose reduced costs fit 32 bits (mcf_small_narrow_fits) runs the front kernel,
//                   k_solve_small<.., true>: 32-bit keys, and the arg-max hands the winner's record to the pivot's begin.
//   k_solve_mid     <= 1 536 nodes: one persistent workgroup over global (L2-resident) state -- prices a Devex
//                   block / re-prices the candidate list / sweeps a small arc list, pivots, permutes, patches.
//                   (both also as k_solve_small_batch / k_solve_mid_batch: MANY independent instances in one launch, one
//                   persistent workgroup = one CU per instance -- mcf_solve_batch)
//   otherwise three kernels per pivot on one stream, 64 pivots per captured hipGraph:
//     k_price_v     Dantzig sweep over 4-BYTE KEY CODES (one per arc, ordering like the violation -state * rc): HBM-bound at
//                   scale, 13.7 us for 16 M arcs; full-sweep Dantzig handles from 4 M arcs on.
//     k_price_rc    the same sweep over RESIDENT reduced costs (8 B rc + 1 B state per arc, +4 B Devex weight):
//                   per-lane best, DPP wave max, one candidate per workgroup.  Devex: the block comes from a granule
//                   table and moves / resizes under the reference's tuner.  Incremental from 4 M arcs: workgroups
//                   whose arcs did not change keep their candidate.
//                   (k_price: the same sweep by gathering pi[tail], pi[head]; mode 0 / parity hook.)
//                   Replaces simplex.py:498-617, simplex_pricing.py:97-137, 310-357, 375-542, simplex_adaptive.py:98-151.
//     k_pivot       one workgroup of 1024: final arg-max over the workgroup candidates (or the candidates
//                   all-gathered from the other ranks), cycle by a workgroup-wide scan over preorder positions
//                   (mcf_pivot_scan; through the coarse index `reach` on large trees; shallow end points are climbed),
//                   ratio test, then mcf_pivot_finish on all lanes (flow update, stem re-parenting, segment table).
//                   Replaces basis.py:178-241, simplex.py:1198-1425.
//     k_update      grid-wide block permutation of the preorder array + potential shift (pi += sigma) + position /
//                   size rewrite + re-indexing of the coarse index, and -- in other workgroups of the same launch --
//                   the patch of the resident reduced costs / key codes of the arcs incident to the re-hung subtree.
//                   Replaces the per-pivot BFS rebuild (basis.py:82-122) and _update_tree_sets (simplex.py:1103-1107).
//
// The host enqueues `batch_pivots` pivots (optionally as one captured hipGraph), then
// reads the small control block back once.  Kernels of a finished solve early-exit.
//
// gfx950 only; no CPU path: without a device every compute entry point returns
// MCF_E_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_core.h"
#include "mcf_host.h"

namespace {

constexpr int kPriceThreads = 256;
constexpr int kPivotThreads = 1024;  // one workgroup: final arg-max, cycle search (climb by one lane / scan by all), finish
constexpr int kReduceThreads = 256;
constexpr int kMidMaxNodes = 1536;           // persistent single-workgroup loop (k_solve_mid): auto up to this many nodes (measured crossover
                                             // with the kernel-per-phase graph: +12..21 % at 512 / 1 024 nodes, even at 2 048, -25 % at 4 096;
                                             // profiles/r02_ab_engine_modes.txt) ...
constexpr int kMidMaxArcsPerPivot = MCF_TUNER_MAX_ARCS + 1024;  // ... and this many arcs priced inside the loop per pivot
constexpr int64_t kIncrementalMinArcs = (int64_t)1 << 22;  // incremental sweeps by default from this many arcs
constexpr int kScanMaxNodes = 1 << 27;  // (with the coarse index the scan's cost no longer grows with the tree: no practical limit)
constexpr int kApplyThreads = 256;
constexpr int kBplMinNodes = 200000;  // blocked preorder list from this many nodes on (auto)
constexpr int kMaxPriceBlocks = 2048;  // 8 workgroups per CU on 256 CUs
constexpr int kMaxApplyBlocks = 512;   // (1 024 workgroups: +5 % in the first 40 K pivots at 1 M nodes, nothing over the whole solve -- 124.5 s either way; MCF_APPLY_BLOCKS, scripts/ab_apply_blocks.py)
#ifndef MCF_PRICE_UNROLL
#define MCF_PRICE_UNROLL 2
#endif
constexpr int kUnroll = MCF_PRICE_UNROLL;  // 4-arc groups in flight per lane in k_price
constexpr int kCtxWords = (int)(sizeof(McfCtx) / 4);   // the control block is staged in LDS word by word

thread_local std::string g_create_error;

// ------------------------------------------------------------------ device helpers
// Wave-wide arg-max of (key, id): max-reduce the 64-bit key with xor shuffles, then resolve the
// id among the lanes that hold the maximum with a ballot + scalar readlanes (almost always one
// lane), instead of shuffling both words through every step.  Result is wave-uniform.
__device__ __forceinline__ int64_t readlane64(int64_t x, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ void wave_argmax(int64_t& key, int64_t& arc) {
    const int64_t mx = mcf_wave_max64(key);  // DPP reduction (mcf_core.h)
    uint64_t mask = __ballot(key == mx && key > 0);
    int64_t best = -1;
    while (mask) {  // uniform loop: one iteration unless several lanes tie on the key
        const int lane = __ffsll((unsigned long long)mask) - 1;
        const int64_t a = readlane64(arc, lane);
        if (best < 0 || a < best) best = a;
        mask &= mask - 1;
    }
    key = best < 0 ? 0 : mx;
    arc = best;
}

// Block-wide arg-max; result valid in thread 0 (and in all of wave 0).
template <int THREADS>
__device__ __forceinline__ void block_argmax(int64_t& key, int64_t& arc) {
    __shared__ int64_t s_key[THREADS / 64];
    __shared__ int64_t s_arc[THREADS / 64];
    wave_argmax(key, arc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_key[wave] = key; s_arc[wave] = arc; }
    __syncthreads();
    if (wave == 0) {
        const bool has = lane < THREADS / 64;
        key = has ? s_key[has ? lane : 0] : 0;
        arc = has ? s_arc[has ? lane : 0] : -1;
        wave_argmax(key, arc);
    }
}

// Block-wide arg-max whose result EVERY wave holds, uniformly (scalar registers): after the one barrier each wave reads all
// the per-wave candidates and reduces them itself, so nobody waits for wave 0 to publish the winner.  The caller keeps a
// barrier between this call and the next (the per-wave slots are rewritten then).
template <int THREADS>
__device__ __forceinline__ void block_argmax_all(int64_t& key, int64_t& arc) {
    __shared__ int64_t s_key[THREADS / 64];
    __shared__ int64_t s_arc[THREADS / 64];
    wave_argmax(key, arc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_key[wave] = key; s_arc[wave] = arc; }
    __syncthreads();   // per-wave candidates -> every wave's reduction over them
    const bool has = lane < THREADS / 64;
    key = has ? s_key[has ? lane : 0] : 0;
    arc = has ? s_arc[has ? lane : 0] : -1;
    wave_argmax(key, arc);
}

// A value every lane of the wave holds alike.  SCALAR: moved to scalar registers (64-bit values in two halves) -- branches on
// it are scalar branches, and it costs no vector register across the loop; !SCALAR: left where the compiler has it.
// (Which of the two the fused LDS loop asks for depends on its width, see small_scalar_control.)
template <bool SCALAR> __device__ __forceinline__ int32_t uni32(int32_t x) {
    if constexpr (SCALAR) return __builtin_amdgcn_readfirstlane(x);
    else return x;
}
template <bool SCALAR> __device__ __forceinline__ int64_t uni64(int64_t x) {
    if constexpr (SCALAR) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
        return (int64_t)(((uint64_t)hi << 32) | lo);
    } else return x;
}
template <bool SCALAR> __device__ __forceinline__ McfNode uni_node(const McfNode& r) {
    return McfNode{uni32<SCALAR>(r.parent), uni32<SCALAR>(r.pred), uni32<SCALAR>(r.size), uni32<SCALAR>(r.depth)};
}

// Candidate cache (McfView::candx): the record of this pricing workgroup's candidate -- end points, state and exact
// reduced cost as of this sweep; the update pass of every following pivot keeps it current.  Thread 0, after the arg-max.
__device__ __forceinline__ void write_candx(const McfView& v, int64_t arc) {
    if (!v.candx) return;
    McfCandX x;
    x.arc = arc; x.rc = 0; x.tail = 0; x.head = 0; x.state = 0; x.pad = 0;
    if (arc >= 0) {
        const int64_t e = arc & 0xffffffff;
        x.tail = v.tail[e]; x.head = v.head[e]; x.state = v.state[e];
        x.rc = (v.rcache && !v.rc_partial) ? v.rcache[e] : (int64_t)v.cost[e] + v.pi[x.tail] - v.pi[x.head];
    }
    v.candx[blockIdx.x] = x;
}

// ------------------------------------------------------------------ k_price
// XCD-aware sweep.  Workgroups are dealt to XCDs round-robin (blockIdx % 8 share an XCD --
// a performance observation, not a correctness assumption), so workgroup b sweeps head-bucket
// b % 8: its random pi[head] gathers stay inside one eighth of the potential array, which the
// XCD's private L2 holds; pi[tail] runs almost sequentially (arcs are tail-sorted inside a
// bucket) and coalesces.  Each lane owns groups of 4 consecutive arcs: one 16-byte load per
// SoA stream (tail, head, cost[, weight]) + 4 state bytes = 13 (17) B per arc.
// Inside the bucket the pass covers the rank's shard and, for Devex, the current block
// (mcf_bucket_slice), both resolved on the device so a captured graph can be replayed.
// FILTER restricts the pass to arcs whose ORIGINAL index lies in [f_lo, f_hi) (parity hook).
template <int RULE, bool FILTER>
__global__ __launch_bounds__(kPriceThreads) void k_price(McfView v, int64_t shard, int64_t shards, int use_block,
                                                          int64_t f_lo, int64_t f_hi, McfCand* __restrict__ cand) {
    int64_t key = 0, arc = -1;
    const McfCtx* c = v.ctx;
    // candidate-list rule: while minor iterations are pending the list of the last sweep must
    // survive, so the whole launch is a no-op (use_block == 2 marks that rule)
    if (use_block == 2 && (c->minor_left > 0 || c->status != MCF_RUNNING)) return;  // (also: a finished batch's
    // trailing launches must not wipe the list a resumed solve will want)
    if (c->status == MCF_RUNNING) {
        const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
        const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
        int64_t lo, hi;
        if (use_block == 1 && v.dx) mcf_devex_slice(v.dx, x, shard, shards, (int32_t)c->block_index, c->block_granules, &lo, &hi);
        else mcf_bucket_slice(v.bucket_off, x, shard, shards, 0, 1, &lo, &hi);
        const int64_t g_lo = lo >> 2, g_hi = (hi + 3) >> 2;  // groups of 4 arcs
        const int4* __restrict__ tail4 = reinterpret_cast<const int4*>(v.tail);
        const int4* __restrict__ head4 = reinterpret_cast<const int4*>(v.head);
        const int4* __restrict__ cost4 = reinterpret_cast<const int4*>(v.cost);
        const int32_t* __restrict__ state4 = reinterpret_cast<const int32_t*>(v.state);
        const float4* __restrict__ w4 = reinterpret_cast<const float4*>(v.weight);
        const int32_t* __restrict__ orig = v.orig;
        const int64_t* __restrict__ pi = v.pi;
        const int64_t stride = nlb * kPriceThreads;
        // kUnroll groups of 4 arcs in flight per lane: all SoA loads are issued first, then all
        // 8 * kUnroll potential gathers, so a wave exposes one memory round trip per phase
        // instead of one per group (the sweep is latency-bound otherwise).
        for (int64_t g0 = g_lo + lb * kPriceThreads + threadIdx.x; g0 < g_hi; g0 += stride * kUnroll) {
            int32_t st[kUnroll];
            int4 t[kUnroll], h[kUnroll], cc[kUnroll];
            float4 w[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t g = g0 + u * stride;
                const bool in = g < g_hi;
                st[u] = in ? state4[g] : 0;
                const int64_t gs = in ? g : g_lo;  // clamp: keep the loads unconditional and in range
                t[u] = tail4[gs];
                h[u] = head4[gs];
                cc[u] = cost4[gs];
                if (RULE == MCF_RULE_DEVEX_BLOCK) w[u] = w4[gs];
            }
            int64_t pt[kUnroll][4], ph[kUnroll][4];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int32_t ts[4] = {t[u].x, t[u].y, t[u].z, t[u].w}, hs[4] = {h[u].x, h[u].y, h[u].z, h[u].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool live = ((st[u] >> (8 * k)) & 0xff) != 0;
                    pt[u][k] = live ? pi[ts[k]] : 0;
                    ph[u][k] = live ? pi[hs[k]] : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int32_t cs[4] = {cc[u].x, cc[u].y, cc[u].z, cc[u].w};
                const float ws[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
                const int64_t g = g0 + u * stride;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int32_t s = (int32_t)(int8_t)(st[u] >> (8 * k));
                    const int64_t i = (g << 2) + k;
                    if (s == 0 || i < lo || i >= hi) continue;
                    const int64_t rc = (int64_t)cs[k] + pt[u][k] - ph[u][k];
                    const int64_t viol = -(int64_t)s * rc;
                    if (viol <= 0) continue;
                    int64_t kk = mcf_dantzig_key(v, i, viol, s);
                    if (RULE == MCF_RULE_DEVEX_BLOCK) {
                        const double merit = ((double)viol * (double)viol) / (double)ws[k];
                        kk = __double_as_longlong(merit);
                    }
                    if (kk < key) continue;              // cannot win: skip the id lookup
                    const int32_t o = orig[i];
                    if (FILTER && (o < f_lo || o >= f_hi)) continue;
                    const int64_t id = mcf_pack_arc(RULE == MCF_RULE_DEVEX_BLOCK ? mcf_devex_tie_id(o, s) : o, i);
                    if (mcf_cand_better(kk, id, key, arc)) { key = kk; arc = id; }
                }
            }
        }
    }
    block_argmax<kPriceThreads>(key, arc);
    if (threadIdx.x == 0) { cand[blockIdx.x] = McfCand{key, arc}; write_candx(v, arc); }
}

// ------------------------------------------------------------------ k_price_rc: sweep over RESIDENT reduced costs
// Large instances keep rc[e] = cost + pi[tail] - pi[head] resident (8 B/arc, exact at all
// times, see k_rcupd).  The sweep is then a pure coalesced stream -- 8 B rc + 1 B state per arc
// (+4 B Devex weight), no gathers, no dependence on the potentials -- instead of 13 B/arc plus
// two random 8-byte gathers that each cost a 128-B L2->L1 line.  Same arc sets (bucket slices),
// same keys, same tie rule as k_price, so it selects the identical entering arc.
template <int RULE, bool FILTER, bool INC>
__global__ __launch_bounds__(kPriceThreads) void k_price_rc(McfView v, int64_t shard, int64_t shards, int use_block,
                                                             int64_t f_lo, int64_t f_hi, McfCand* __restrict__ cand,
                                                             int64_t* __restrict__ swept, const int32_t* __restrict__ blk_tab) {
    // On small and mid-size instances this kernel is a latency chain (control block -> arc data -> ids -> arg-max),
    // so: (1) the first batch of arc data is requested BEFORE the control block is looked at (full sweeps: the
    // slice does not depend on it); (2) the caller's arc id, needed only to break ties and to name the winner, is
    // looked up once per lane at the end instead of once per improvement.
    const McfCtx* c = v.ctx;
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    using rc2_t = long2;                                  // two int64 reduced costs per 16-byte load
    const rc2_t* __restrict__ rc2 = reinterpret_cast<const rc2_t*>(v.rcache);
    const int32_t* __restrict__ state4 = reinterpret_cast<const int32_t*>(v.state);
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(v.weight);
    const int32_t* __restrict__ orig = v.orig;
    const int64_t stride = nlb * kPriceThreads;
    constexpr int U = 4;
    int32_t st[U];
    rc2_t ra[U], rb[U];
    float4 w[U];
    int64_t lo = 0, hi = 0, g_lo = 0, g_hi = 0;
    auto load_batch = [&](int64_t g0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t g = g0 + u * stride;
            const bool in = g < g_hi;
            const int64_t gs = in ? g : g_lo;  // clamp: keep the loads unconditional and in range
            st[u] = in ? state4[gs] : 0;
            ra[u] = rc2[2 * gs];
            rb[u] = rc2[2 * gs + 1];
            if (RULE == MCF_RULE_DEVEX_BLOCK) w[u] = w4[gs];
        }
    };
    const bool early = use_block != 1;  // full sweep: the slice is known without the control block
    int64_t g0 = 0;
    if (early) {
        // this rank's share of bucket x: a host-made table when the arc list is sharded (divisions otherwise)
        if (blk_tab) { lo = blk_tab[x * 2]; hi = blk_tab[x * 2 + 1]; }
        else mcf_bucket_slice(v.bucket_off, x, shard, shards, 0, 1, &lo, &hi);
        g_lo = lo >> 2; g_hi = (hi + 3) >> 2;  // groups of 4 arcs
        g0 = g_lo + lb * kPriceThreads + threadIdx.x;
        if (g0 < g_hi) load_batch(g0);
    }
    // candidate-list rule: while minor iterations are pending the list of the last sweep must
    // survive, so the whole launch is a no-op (use_block == 2 marks that rule)
    if (use_block == 2 && (c->minor_left > 0 || c->status != MCF_RUNNING)) return;  // (also: a finished batch's
    // trailing launches must not wipe the list a resumed solve will want)
    // incremental full sweep: no arc of this block changed since the block was last swept -> cand[blockIdx.x] still
    // holds.  (A finished batch's trailing launches must leave the candidates alone too: a resumed solve relies on them.)
    if (INC && v.dirty && use_block != 1 && (c->status != MCF_RUNNING || !v.dirty->flag[blockIdx.x])) return;
    int64_t key = 0, arc = -1;
    int64_t best_i = -1;  // engine index of this lane's best arc (its caller's id is looked up at the end)
    int32_t best_s = 0;   // its state (Devex: the direction takes part in the tie rule)
    if (c->status == MCF_RUNNING) {
        if (!early) {
            // Devex block search: this rank's share of block k of bucket x, from the host-made granule table (two
            // dependent 4-byte loads; the block size changes under the tuner, so blocks themselves cannot be tabulated)
            if (v.dx) mcf_devex_slice(v.dx, x, shard, shards, (int32_t)c->block_index, c->block_granules, &lo, &hi);
            else mcf_bucket_slice(v.bucket_off, x, shard, shards, 0, 1, &lo, &hi);
            g_lo = lo >> 2; g_hi = (hi + 3) >> 2;
            g0 = g_lo + lb * kPriceThreads + threadIdx.x;
            if (g0 < g_hi) load_batch(g0);
        }
        if (INC && swept && threadIdx.x == 0) {
            // accounting off the critical path: 32-bit arithmetic, and a no-return atomic on the workgroup's private slot
            // (nothing waits for it; one shared word would serialise 2 048 atomics, ~10 us per sweep).
            // This workgroup's share of the slice: groups g_lo + lb * 256 + [0, 256) + j * nlb * 256.
            const uint32_t ng = (uint32_t)(g_hi - g_lo), per = (uint32_t)nlb * 256u, full = ng / per, rem = ng - full * per;
            const uint32_t off = (uint32_t)lb * 256u;
            const uint32_t mine = full * 256u + (rem > off ? (rem - off < 256u ? rem - off : 256u) : 0u);
            atomicAdd(reinterpret_cast<unsigned long long*>(swept) + blockIdx.x, (unsigned long long)mine * 4ull);
        }
        while (g0 < g_hi) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t rcs[4] = {ra[u].x, ra[u].y, rb[u].x, rb[u].y};
                const float ws[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
                const int64_t g = g0 + u * stride;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int32_t s = (int32_t)(int8_t)(st[u] >> (8 * k));
                    const int64_t i = (g << 2) + k;
                    if (s == 0 || i < lo || i >= hi) continue;
                    const int64_t viol = -(int64_t)s * rcs[k];
                    if (viol <= 0) continue;
                    int64_t kk = mcf_dantzig_key(v, i, viol, s);
                    if (RULE == MCF_RULE_DEVEX_BLOCK) {
                        const double merit = ((double)viol * (double)viol) / (double)ws[k];
                        kk = __double_as_longlong(merit);
                    }
                    if (kk < key) continue;
                    if (FILTER) {  // parity hook: the caller's index range decides eligibility
                        const int32_t o = orig[i];
                        if (o < f_lo || o >= f_hi) continue;
                    }
                    if (kk > key) { key = kk; best_i = i; best_s = s; }
                    else if (best_i < 0) { best_i = i; best_s = s; }
                    else {  // tie on the key (rare): Devex prefers a backward arc, then the lowest caller's index
                        const int32_t a = RULE == MCF_RULE_DEVEX_BLOCK ? mcf_devex_tie_id(orig[i], s) : orig[i];
                        const int32_t b = RULE == MCF_RULE_DEVEX_BLOCK ? mcf_devex_tie_id(orig[best_i], best_s) : orig[best_i];
                        if (a < b) { best_i = i; best_s = s; }
                    }
                }
            }
            g0 += stride * U;
            if (g0 < g_hi) load_batch(g0);
        }
        if (best_i >= 0) arc = mcf_pack_arc(RULE == MCF_RULE_DEVEX_BLOCK ? mcf_devex_tie_id(orig[best_i], best_s) : orig[best_i], best_i);
    }
    block_argmax<kPriceThreads>(key, arc);
    if (threadIdx.x == 0) {
        cand[blockIdx.x] = McfCand{key, arc};
        write_candx(v, arc);
        // every lane has passed the gate above (the arg-max has a barrier): the flag may go down now
        if (INC && v.dirty && use_block != 1 && c->status == MCF_RUNNING) v.dirty->flag[blockIdx.x] = 0;
    }
}

// ------------------------------------------------------------------ k_price_v: Dantzig sweep over COMPRESSED keys
// 4 bytes per arc (McfView::vkey, see mcf_core.h) instead of 8 B reduced cost + 1 B state: the sweep is HBM-bound at
// scale, so bytes are time.  Same arc sets, same arg-max, same tie rule as k_price_rc<DANTZIG>: a code orders like the
// violation it stands for and equal codes mean equal violations; an arc whose violation does not fit the code
// (MCF_VKEY_SAT) is compared by its exact value, fetched on the spot.  The workgroup's candidate carries the exact
// violation (one look-up per lane at the end, together with the caller's arc id), so k_pivot / k_reduce see what
// they always saw.
// NT: the code stream is loaded with the non-temporal hint -- for sweeps larger than the Infinity Cache, where no line
// is ever re-used before it is evicted (below that size the next sweep re-reads the lines from the cache: no hint).
template <bool INC, bool NT = false>
__global__ __launch_bounds__(kPriceThreads) void k_price_v(McfView v, int64_t shard, int64_t shards, int use_block,
                                                            McfCand* __restrict__ cand, int64_t* __restrict__ swept,
                                                            const int32_t* __restrict__ blk_tab) {
    const McfCtx* c = v.ctx;
    const int x = blockIdx.x & (MCF_NUM_BUCKETS - 1);
    const int64_t lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int4* __restrict__ vk4 = reinterpret_cast<const int4*>(v.vkey);
    const int32_t* __restrict__ orig = v.orig;
    const int64_t stride = nlb * kPriceThreads;
    constexpr int U = 8;   // 16-byte loads in flight per lane (4 arcs each)
    int4 q[U];
    int64_t lo, hi;
    if (blk_tab) { lo = blk_tab[x * 2]; hi = blk_tab[x * 2 + 1]; }
    else mcf_bucket_slice(v.bucket_off, x, shard, shards, 0, 1, &lo, &hi);
    const int64_t g_lo = lo >> 2, g_hi = (hi + 3) >> 2;  // groups of 4 arcs
    auto load_batch = [&](int64_t g0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t g = g0 + u * stride;
            if (g >= g_hi) q[u] = make_int4(0, 0, 0, 0);
            else if (NT) {
                typedef int nt_int4 __attribute__((ext_vector_type(4)));
                const nt_int4 w = __builtin_nontemporal_load(reinterpret_cast<const nt_int4*>(vk4) + g);
                q[u] = make_int4(w.x, w.y, w.z, w.w);
            } else q[u] = vk4[g];
        }
    };
    int64_t g0 = g_lo + lb * kPriceThreads + threadIdx.x;
    if (g0 < g_hi) load_batch(g0);   // before the control block is looked at: a full sweep's slice does not depend on it
    if (use_block == 2 && (c->minor_left > 0 || c->status != MCF_RUNNING)) return;   // candidate list still live
    if (INC && v.dirty && (c->status != MCF_RUNNING || !v.dirty->flag[blockIdx.x])) return;  // clean block: candidate stands
    int32_t best = 0;      // best code of this lane (MCF_VKEY_SAT: its violation is not coded, best_x holds it)
    int64_t best_i = -1;   // its engine arc
    int64_t best_x = 0;    // exact violation while best == MCF_VKEY_SAT
    const int64_t bigm = v.vk_bigm;
    const int32_t half = v.vk_half;
    auto exact = [&](int64_t i) { return -(int64_t)v.state[i] * v.rcache[i]; };
    if (c->status == MCF_RUNNING) {
        if (INC && swept && threadIdx.x == 0) {
            const uint32_t ng = (uint32_t)(g_hi - g_lo), per = (uint32_t)nlb * 256u, full = ng / per, rem = ng - full * per;
            const uint32_t off = (uint32_t)lb * 256u;
            const uint32_t mine = full * 256u + (rem > off ? (rem - off < 256u ? rem - off : 256u) : 0u);
            atomicAdd(reinterpret_cast<unsigned long long*>(swept) + blockIdx.x, (unsigned long long)mine * 4ull);
        }
        while (g0 < g_hi) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t ks[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                const int64_t g = g0 + u * stride;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int32_t kk = ks[k];
                    if (kk == 0 || (kk < best && best != MCF_VKEY_SAT)) continue;   // ineligible / cannot win
                    const int64_t i = (g << 2) + k;
                    if (i < lo || i >= hi) continue;
                    if (kk != MCF_VKEY_SAT && best != MCF_VKEY_SAT) {   // the common case: codes order like violations
                        if (kk > best) { best = kk; best_i = i; }
                        else if (orig[i] < orig[best_i]) best_i = i;    // equal codes = equal violations: lowest caller's index
                    } else {                                             // an arc that is not coded is involved: exact values
                        const int64_t xv = kk == MCF_VKEY_SAT ? exact(i) : mcf_vkey_decode(kk, bigm, half);
                        const int64_t cur = best_i < 0 ? 0 : (best == MCF_VKEY_SAT ? best_x : mcf_vkey_decode(best, bigm, half));
                        if (xv > cur || (xv == cur && best_i >= 0 && orig[i] < orig[best_i])) { best = kk; best_i = i; best_x = xv; }
                    }
                }
            }
            g0 += stride * U;
            if (g0 < g_hi) load_batch(g0);
        }
    }
    int64_t key = 0, arc = -1;
    if (best_i >= 0) {
        key = best == MCF_VKEY_SAT ? best_x : mcf_vkey_decode(best, bigm, half);   // the exact violation, as k_price_rc reports it
        arc = mcf_pack_arc(orig[best_i], best_i);
    }
    block_argmax<kPriceThreads>(key, arc);
    if (threadIdx.x == 0) {
        cand[blockIdx.x] = McfCand{key, arc};
        write_candx(v, arc);
        if (INC && v.dirty && c->status == MCF_RUNNING) v.dirty->flag[blockIdx.x] = 0;
    }
}

// ------------------------------------------------------------------ keeping the resident reduced costs exact
// The swap shifted the potentials of the re-hung subtree T2 by sigma, so an arc changes iff exactly
// one end point is in T2: +sigma when its tail is inside, -sigma when its head is.  16 lanes per T2
// node walk its CSR adjacency; every such arc is visited exactly once (from its inside end), so no
// atomics.  The pass lives in k_update below.
constexpr int kRcupdThreads = 256;
constexpr int kMaxRcupdBlocks = 1024;
constexpr int kCandxBlocks = 8;   // workgroups of the dense update launches that keep the candidate cache current (2 048 entries)

// ------------------------------------------------------------------ k_update = tree/potential apply + reduced-cost update in ONE launch
// Resident-rc engines only.  The two halves touch disjoint data once T2 membership is tested
// against the OLD positions (posbuf[cur], which this launch never writes) and T2 is enumerated
// through the OLD order (order[cur][a0 .. a0+S)): the apply half writes order[cur^1],
// posbuf[cur^1], pi and the depths of T2; the update half writes rcache.  One launch boundary less per pivot.
// `c` is the control block (kernel argument memory / LDS); the pass is spread over `stride` lanes of which this
// one is `tid`, and over `ngroups` 16-lane groups of which this lane belongs to `group` (sub-lane `sub`).
__device__ __forceinline__ int32_t wave_max32(int32_t x) { return (int32_t)mcf_wave_max64((int64_t)x); }  // DPP steps, no LDS crossbar

// `tid` of `stride` lanes, both multiples of 64 apart: whole waves.  With a coarse index (v.reach) every wave takes
// aligned blocks of 64 positions, so that it holds all 64 new subtree sizes of a block and re-indexes reach[] in the
// same pass (one wave max + one store per block).
__device__ __forceinline__ void apply_pass(const McfView& v, const McfCtx& c, int64_t tid, int64_t stride) {
    const int32_t lo = c.lo, hi = c.hi, plo = c.prev_lo, phi = c.prev_hi;
    if (!v.reach) {
        for (int64_t j = lo + tid; j < hi; j += stride) mcf_apply_one(v, c, (int32_t)j);
        for (int64_t j = plo + tid; j < phi; j += stride)
            if (j < lo || j >= hi) mcf_apply_one(v, c, (int32_t)j);
        return;
    }
    const int32_t* zsrc = c.cur ? v.psz[1] : v.psz[0];  // the stable old view (outside [lo, hi) old == new)
    const int32_t lane = (int32_t)(tid & 63);
    const int64_t gw = tid >> 6, nw = stride >> 6;
    const int32_t B0 = lo >> MCF_REACH_SHIFT, B1 = hi > lo ? (hi - 1) >> MCF_REACH_SHIFT : B0 - 1;
    const int32_t P0 = plo >> MCF_REACH_SHIFT, P1 = phi > plo ? (phi - 1) >> MCF_REACH_SHIFT : P0 - 1;
    // Up to KB blocks of a wave are permuted first and re-indexed afterwards: the sizes a block's re-indexing needs are
    // loaded by the permutation itself, and using them right away would make every block wait for its own loads
    // (measured at 1 M nodes: k_update 8.6 -> 11.1 us); deferred, the loads of all KB blocks are in flight together.
    constexpr int KB = 4;
    auto blocks = [&](int64_t first, int64_t last, int64_t skip_lo, int64_t skip_hi) {
        for (int64_t b0 = first + gw; b0 <= last; b0 += nw * KB) {
            int32_t z[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const int64_t b = b0 + k * nw;
                z[k] = 0;
                if (b > last || (b >= skip_lo && b <= skip_hi)) continue;   // (wave-uniform)
                const int32_t j = ((int32_t)b << MCF_REACH_SHIFT) + lane;
                if (j < v.n_nodes) {
                    const bool in_cur = j >= lo && j < hi, in_prev = j >= plo && j < phi;
                    z[k] = (in_cur || in_prev) ? mcf_apply_one(v, c, j) : zsrc[j];
                }
            }
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const int64_t b = b0 + k * nw;
                if (b > last || (b >= skip_lo && b <= skip_hi)) continue;
                const int32_t j = ((int32_t)b << MCF_REACH_SHIFT) + lane;
                const int32_t m = wave_max32(j < v.n_nodes ? j + z[k] : 0);
                if (lane == 0) v.reach[b] = m;
            }
        }
    };
    blocks(B0, B1, 1, 0);        // the moved range
    blocks(P0, P1, B0, B1);      // the catch-up range, minus what the first call covered
    // shrunken subtrees outside both ranges: their blocks from the stable view (the finish pass wrote the new sizes
    // into both copies)
    for (int64_t t = gw; t < c.nchg; t += nw) {
        const int32_t b = v.chg[t] >> MCF_REACH_SHIFT;
        if ((b < B0 || b > B1) && (b < P0 || b > P1)) {
            const int32_t j = (b << MCF_REACH_SHIFT) + lane;
            const int32_t m = wave_max32(j < v.n_nodes ? j + zsrc[j] : 0);
            if (lane == 0) v.reach[b] = m;
        }
    }
}

__device__ __forceinline__ void rcupd_pass(const McfView& v, const McfCtx& c, int64_t group, int64_t ngroups, int32_t sub) {
    if (!v.rcache) return;
    const int32_t a0 = c.t2_old, S = c.t2_size;
    const int64_t sigma = c.sigma;
    const int32_t* __restrict__ ord = c.cur ? v.order[1] : v.order[0];     // old order
    const int32_t* __restrict__ pold = c.cur ? v.posbuf[1] : v.posbuf[0];  // old positions
    const int64_t* __restrict__ adj_off = v.adj_off;
    const int64_t* __restrict__ adj = v.adj;
    int64_t* __restrict__ rcache = v.rcache;
    if (c.pv_t2n == 1) {
        // [r3] T2 is the one node the pivot kernel named, and its adjacency range came along with the control block: control
        // block -> adjacency -> reduced cost, instead of -> order -> adjacency offsets -> adjacency -> other end's position ->
        // reduced cost (the longest chain of the launch on the first pivots of a cold start, when almost every T2 is one node)
        if (group != 0) return;
        const int32_t node = c.pv_t2node;
        for (int64_t p = c.pv_adj[0] + sub; p < c.pv_adj[1]; p += 16) {
            const int64_t ent = adj[p];
            if ((int32_t)(ent >> 32) == node) continue;  // a loop: both ends inside T2
            const int32_t e = (int32_t)((uint32_t)ent >> 1);
            const int64_t r = rcache[e] + ((ent & 1) ? sigma : -sigma);
            rcache[e] = r;
            if (v.vkey) v.vkey[e] = mcf_vkey(-(int64_t)v.state[e] * r, v.vk_bigm, v.vk_half);
            mcf_mark_dirty(v, e);
        }
        return;
    }
    for (int64_t t = group; t < S; t += ngroups) {
        const int32_t u = ord[a0 + t];
        const int64_t beg = adj_off[u], end = adj_off[u + 1];
        for (int64_t p = beg + sub; p < end; p += 16) {
            const int64_t ent = adj[p];
            const int32_t pw = pold[(int32_t)(ent >> 32)];
            if (pw >= a0 && pw < a0 + S) continue;  // both ends inside T2: unchanged
            const int32_t e = (int32_t)((uint32_t)ent >> 1);
            const int64_t r = rcache[e] + ((ent & 1) ? sigma : -sigma);
            rcache[e] = r;
            // the compressed key follows (the finish pass has already given the entering / leaving arc its new state)
            if (v.vkey) v.vkey[e] = mcf_vkey(-(int64_t)v.state[e] * r, v.vk_bigm, v.vk_half);
            mcf_mark_dirty(v, e);
        }
    }
}

// Candidate cache: every listed arc's reduced cost follows the potential shift of the re-hung subtree (+sigma when its tail
// is inside T2, -sigma when its head is), and the leaving arc's entry takes its new state.  Membership against the OLD view,
// like the reduced-cost patch; a single-node T2 whose node the pivot kernel named needs no look-up at all.
__device__ __forceinline__ void candx_pass(const McfView& v, const McfCtx& c, int32_t tid, int32_t stride) {
    if (!v.candx) return;
    const bool bpl = MCF_HAS_BPL(v);
    const int32_t a0 = c.t2_old, S = c.t2_size;
    const int32_t* __restrict__ pold = c.cur ? v.posbuf[1] : v.posbuf[0];  // dense array: old positions
    const bool one = c.pv_t2n == 1;   // (either layout)
    for (int32_t i = tid; i < v.ncandx; i += stride) {
        McfCandX x = v.candx[i];
        if (x.arc < 0) continue;
        bool tin, hin;
        if (one) { tin = x.tail == c.pv_t2node; hin = x.head == c.pv_t2node; }
        else if (bpl) { tin = mcf_bpl_in_t2(v, c, x.tail); hin = mcf_bpl_in_t2(v, c, x.head); }
        else { const int32_t pt = pold[x.tail], ph = pold[x.head]; tin = pt >= a0 && pt < a0 + S; hin = ph >= a0 && ph < a0 + S; }
        const bool leave = (int32_t)(x.arc & 0xffffffff) == c.pv_leave;
        if (tin == hin && !leave) continue;
        if (tin != hin) x.rc += tin ? c.sigma : -c.sigma;
        if (leave) x.state = c.pv_leave_state;
        v.candx[i] = x;
    }
}

// The two halves are independent, and each is a chain of dependent loads: different workgroups run them side
// by side (the first `apply_blocks` the permutation, the others the reduced-cost patch) instead of one after the other.
template <bool MARK>  // MARK: the handle prices incrementally, the patched arcs' blocks are flagged
__global__ __launch_bounds__(kRcupdThreads) void k_update(McfView g, int apply_blocks) {
    McfView v = g;
    if (!MARK) v.dirty = nullptr;  // folds the marking away
    const McfCtx c = *v.ctx;  // uniform: scalar loads
    if (!c.apply) return;
    const int b = blockIdx.x;
    const int xb = v.candx ? kCandxBlocks : 0;   // the last workgroups keep the candidate cache current
    if (b < apply_blocks) {
        apply_pass(v, c, (int64_t)b * kRcupdThreads + threadIdx.x, (int64_t)apply_blocks * kRcupdThreads);
    } else if (b >= (int)gridDim.x - xb) {
        candx_pass(v, c, (b - ((int)gridDim.x - xb)) * kRcupdThreads + (int)threadIdx.x, xb * kRcupdThreads);
    } else {
        const int64_t rb = b - apply_blocks, nrb = (int64_t)gridDim.x - apply_blocks - xb;
        rcupd_pass(v, c, rb * (kRcupdThreads / 16) + (threadIdx.x >> 4), nrb * (kRcupdThreads / 16), threadIdx.x & 15);
    }
}


// ------------------------------------------------------------------ k_update_bpl: the update over the BLOCKED preorder list
// (mcf_core.h "blocked preorder list").  Workgroups 0 .. G-1, three phases:
//   A  one lane per physical block handed out before this pivot (block b belongs to workgroup b % G, so that the
//      consecutive blocks of a large subtree spread over the grid): read {base, rrel} and the live range, write the record's
//      new copy -- for almost every block just base + shift -- or list the block as one to take apart;
//   B  one wave per listed block, one lane per slot: T2's elements go to their new blocks (segment table, potential and
//      depth shift on the way), cut-off runs to the copy blocks, the block's records are rewritten; the T2 nodes met are
//      listed in LDS;
//   C  16 lanes per listed T2 node walk its adjacency and patch the resident reduced costs / key codes of the arcs whose
//      other end is outside T2 (mcf_bpl_in_t2: valid whether or not that node has been moved yet).
// Workgroup G (the DIRECT one) skips A: the pivot kernel already knows two blocks that have to be taken apart -- the one T2
// starts in and the new parent's -- so this workgroup starts on them the moment the control block has arrived, with the
// segment table in LDS.  Almost every pivot re-hangs a handful of nodes that sit in that one block: then the whole launch
// is   control block -> slots -> adjacency offsets -> adjacency -> reduced costs   (five dependent round trips), and the
// membership test of the patch is a look-up in the LDS list instead of two more loads per arc.
// With ctx.rebuild every block is taken apart (no direct workgroup) and every element lands at slot = new position in the
// other arena.
constexpr int kBplThreads = 1024;
constexpr int kBplTouchedCap = 2048;   // blocks one workgroup can list (mcf_create sizes the grid so that a workgroup owns no more)
constexpr int kBplT2Cap = 8192;        // T2 nodes one workgroup can list (more: patched on the spot by the lane that moved them)
constexpr int kBplSegLds = 1024;       // segment-table entries a workgroup stages in LDS (one per thread) before it moves T2 elements
constexpr int kBplListMember = 32;     // a T2 this small that sits in one block: membership by scanning the LDS list

// `whole` != null: the listed nodes are ALL of T2 (n of them): the other end is inside iff it is in the list
template <bool MARK>
__device__ __forceinline__ void bpl_patch_node(const McfView& v, const McfCtx& c, int32_t u, int32_t sub, int32_t nsub,
                                               const int32_t* whole = nullptr, int32_t n = 0) {
    const int64_t sigma = c.sigma;
    const int64_t beg = v.adj_off[u], end = v.adj_off[u + 1];
    int64_t* __restrict__ rcache = v.rcache;
    for (int64_t p = beg + sub; p < end; p += nsub) {
        const int64_t ent = v.adj[p];
        const int32_t other = (int32_t)(ent >> 32);
        bool inside;
        if (whole) { inside = false; for (int32_t q = 0; q < n; ++q) inside |= whole[q] == other; }
        else inside = mcf_bpl_in_t2(v, c, other);
        if (inside) continue;  // both ends inside T2: unchanged
        const int32_t e = (int32_t)((uint32_t)ent >> 1);
        const int64_t r = rcache[e] + ((ent & 1) ? sigma : -sigma);
        rcache[e] = r;
        if (v.vkey) v.vkey[e] = mcf_vkey(-(int64_t)v.state[e] * r, v.vk_bigm, v.vk_half);
        if (MARK) mcf_mark_dirty(v, e);
    }
}

// One wave takes block b apart (phase B).  `segv`: the view with the segment table wherever it is cheapest to search.
template <bool MARK, bool RC>
__device__ __forceinline__ void bpl_block(const McfView& v, const McfView& segv, const McfCtx& c, McfCtx* gctx, int32_t b, int32_t lane,
                                          int32_t* s_t2, int32_t* s_nn, bool list = true, int32_t t2_cap = kBplT2Cap) {
    const int32_t bs = v.blk_shift;
    const McfBlkMeta* __restrict__ bm = c.cur ? v.bmeta[1] : v.bmeta[0];
    McfBlkMeta* __restrict__ bn = c.cur ? v.bmeta[0] : v.bmeta[1];
    int32_t* __restrict__ xa = c.arena ? v.bext[1] : v.bext[0];
    const int32_t* __restrict__ tok = c.arena ? v.order[1] : v.order[0];
    const int32_t* __restrict__ psz = c.arena ? v.psz[1] : v.psz[0];
    // the slots are requested together with the block's record (they do not depend on it): one round trip
    constexpr int kChunks = 4;   // 64-slot chunks held in registers (blocks up to 256 slots; larger ones loop on)
    int32_t zr[kChunks], nr[kChunks];
#pragma unroll
    for (int q = 0; q < kChunks; ++q) {
        const int32_t o = q * 64 + lane;
        const bool in = o < (1 << bs);
        zr[q] = in ? psz[(b << bs) + o] : 0;
        nr[q] = in ? tok[(b << bs) + o] : 0;
    }
    const McfBlkMeta m = bm[b];
    const int32_t x = xa[b], beg = mcf_ext_beg(x), end = mcf_ext_end(x);
    if (m.base == MCF_BLK_FREE || end <= beg) { if (!c.rebuild && lane == 0) bn[b] = McfBlkMeta{MCF_BLK_FREE, 0}; return; }
    const McfBlkPlan P = mcf_bpl_plan(c, m.base, m.base + beg, m.base + end);
    if (!c.rebuild && !P.touched && !(x & MCF_EXT_FLAG)) { if (lane == 0) bn[b] = McfBlkMeta{P.nbase, m.rrel}; return; }
    const bool reindex_only = !c.rebuild && !P.touched;
    int32_t keep = 0, cr0 = 0, cr1 = 0;
    for (int32_t o0 = beg & ~63; o0 < end; o0 += 64) {
        const int32_t o = o0 + lane, q = o0 >> 6;
        int32_t pblk = -1, pval = 0;   // this lane's pushed element: destination block and o + z there
        if (o >= beg && o < end) {
            const int32_t slot = (b << bs) + o;
            int32_t z, nd;
            if (q < kChunks) { z = q == 0 ? zr[0] : (q == 1 ? zr[1] : (q == 2 ? zr[2] : zr[3])); nd = q == 0 ? nr[0] : (q == 1 ? nr[1] : (q == 2 ? nr[2] : nr[3])); }
            else { z = psz[slot]; nd = tok[slot]; }
            if (reindex_only) { keep = keep > o + z ? keep : o + z; }
            else {
                const int32_t p = m.base + o;
                McfBplOut r;
                mcf_bpl_slot(segv, c, P, slot, p, nd, z, &r);
                pblk = r.push_blk; pval = r.push_reach;
                keep = keep > r.keep_reach ? keep : r.keep_reach;
                cr0 = cr0 > r.copy_reach[0] ? cr0 : r.copy_reach[0];
                cr1 = cr1 > r.copy_reach[1] ? cr1 : r.copy_reach[1];
                if (RC && list && p >= c.t2_old && p < c.t2_old + c.t2_size) {
                    const int32_t li = atomicAdd(s_nn, 1);
                    if (li < t2_cap) s_t2[li] = nd;
                    else bpl_patch_node<MARK>(v, c, nd, 0, 1);   // list full: this lane patches the node's arcs itself
                }
            }
        }
        // the pushed elements raise the rrel of the blocks they land in: one atomic per destination block and chunk (consecutive
        // old positions mostly land in one or two blocks), not one per element -- thousands of them on a few dozen words otherwise
        for (uint64_t todo = __ballot(pblk >= 0); todo;) {
            const int32_t b0 = __builtin_amdgcn_readlane(pblk, (int)__ffsll((unsigned long long)todo) - 1);
            const bool mine = pblk == b0;
            const int32_t mx = wave_max32(mine ? pval : 0);
            if (lane == 0) atomicMax(&bn[b0].rrel, mx);
            todo &= ~__ballot(mine);
        }
    }
    if (c.rebuild) return;   // (the old arena is left empty; its records die with the flip)
    keep = wave_max32(keep); cr0 = wave_max32(cr0); cr1 = wave_max32(cr1);
    if (lane == 0) {
        bn[b] = McfBlkMeta{P.nbase, keep};
        xa[b] = P.nbase == MCF_BLK_FREE ? 0 : mcf_ext_make(P.r0lo - m.base, P.r0hi - m.base);
        int32_t nm = 0;
#pragma unroll
        for (int kd = 0; kd < 2; ++kd) {
            const int32_t ilo = kd ? P.ilo[1] : P.ilo[0], ihi = kd ? P.ihi[1] : P.ihi[0];
            if (ihi <= ilo) continue;
            const int32_t cb = c.alloc_lo + kd;
            bn[cb] = McfBlkMeta{ilo + mcf_bpl_shift(c, ilo), kd ? cr1 : cr0};
            xa[cb] = mcf_ext_make(0, ihi - ilo);
            nm += ihi - ilo;
        }
        if (nm) atomicAdd(reinterpret_cast<unsigned long long*>(&gctx->nodes_moved), (unsigned long long)nm);
    }
}

template <bool MARK, bool RC>
__global__ __launch_bounds__(kBplThreads) void k_update_bpl(McfView g, int G) {
    __shared__ McfCtx cs;
    __shared__ int32_t s_nt, s_nn;
    __shared__ int32_t s_tb[kBplTouchedCap];
    __shared__ int32_t s_t2[RC ? kBplT2Cap : 1];
    __shared__ McfSeg s_seg[kBplSegLds];
    const bool direct = (int32_t)blockIdx.x == G;
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(&cs)[threadIdx.x] = reinterpret_cast<const int32_t*>(g.ctx)[threadIdx.x];
    // the direct workgroup will search the segment table for sure: it fetches it together with the control block (the scratch
    // holds 2 n + 2 entries: reading the first 64 is always in bounds; longer tables are staged below, once nseg is known)
    if (direct && threadIdx.x >= 128 && threadIdx.x < 128 + 64) s_seg[threadIdx.x - 128] = g.seg[threadIdx.x - 128];
    if (threadIdx.x == 0) { s_nt = 0; s_nn = 0; }
    __syncthreads();
    const McfCtx& c = cs;
    if (!c.apply) return;
    McfView v = g;
    if (!MARK) v.dirty = nullptr;
    if ((int32_t)blockIdx.x > G) { candx_pass(v, c, (int32_t)threadIdx.x, kBplThreads); return; }   // the candidate cache's workgroup
    const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t known0 = c.rebuild ? -1 : c.t2_blk, known1 = c.rebuild ? -1 : c.ins_blk;   // taken apart by the direct workgroup
    if (direct) {
        if (c.rebuild) return;
        McfView segv = v;
        if (c.nseg > 64 && c.nseg <= kBplSegLds) {   // (uniform) a longer table: the rest of it, one entry per thread
            if ((int32_t)threadIdx.x >= 64 && (int32_t)threadIdx.x < c.nseg) s_seg[threadIdx.x] = g.seg[threadIdx.x];
            __syncthreads();
        }
        if (c.nseg <= kBplSegLds) segv.seg = s_seg;
        if (RC && c.pv_t2n == 1) {
            // T2 is one node and the pivot kernel sent its adjacency range along: the patch needs no look-up at all
            // (control block -> adjacency -> reduced costs); the node has no arc to itself, so every incident arc changes
            if (wave == 0) bpl_block<MARK, false>(v, segv, c, g.ctx, known0, lane, s_t2, &s_nn);
            else if (wave == 1 && known1 >= 0 && known1 != known0) bpl_block<MARK, false>(v, segv, c, g.ctx, known1, lane, s_t2, &s_nn);
            else if (wave >= 2) {
                const int64_t sigma = c.sigma;
                for (int64_t p = c.pv_adj[0] + (threadIdx.x - 128); p < c.pv_adj[1]; p += kBplThreads - 128) {
                    const int64_t ent = v.adj[p];
                    const int32_t e = (int32_t)((uint32_t)ent >> 1);
                    const int64_t r = v.rcache[e] + ((ent & 1) ? sigma : -sigma);
                    v.rcache[e] = r;
                    if (v.vkey) v.vkey[e] = mcf_vkey(-(int64_t)v.state[e] * r, v.vk_bigm, v.vk_half);
                    if (MARK) mcf_mark_dirty(v, e);
                }
            }
            return;
        }
        if (wave == 0) bpl_block<MARK, RC>(v, segv, c, g.ctx, known0, lane, s_t2, &s_nn);
        else if (wave == 1 && known1 >= 0 && known1 != known0) bpl_block<MARK, RC>(v, segv, c, g.ctx, known1, lane, s_t2, &s_nn);
        if (!RC) return;
        __syncthreads();
        const int32_t nn = s_nn < kBplT2Cap ? s_nn : kBplT2Cap;
        const bool whole = nn == c.t2_size && nn <= kBplListMember;   // all of T2 sat in the known block
        for (int32_t t = threadIdx.x >> 4; t < nn; t += kBplThreads / 16)
            bpl_patch_node<MARK>(v, c, s_t2[t], threadIdx.x & 15, 16, whole ? s_t2 : nullptr, nn);
        return;
    }
    const McfBlkMeta* __restrict__ bm = c.cur ? v.bmeta[1] : v.bmeta[0];
    McfBlkMeta* __restrict__ bn = c.cur ? v.bmeta[0] : v.bmeta[1];
    const int32_t* __restrict__ xa = c.arena ? v.bext[1] : v.bext[0];
    const int32_t nold = c.alloc_prev;
    // ---- A
    for (int32_t q = threadIdx.x;; q += kBplThreads) {
        const int32_t b = q * G + (int32_t)blockIdx.x;
        if (b >= nold) break;
        if (b == known0 || b == known1) continue;
        const McfBlkMeta m = bm[b];
        const int32_t x = xa[b], beg = mcf_ext_beg(x), end = mcf_ext_end(x);
        if (m.base == MCF_BLK_FREE || end <= beg) { if (!c.rebuild) bn[b] = McfBlkMeta{MCF_BLK_FREE, 0}; continue; }
        bool apart = c.rebuild != 0 || (x & MCF_EXT_FLAG) != 0;
        if (!apart) {
            const McfBlkPlan P = mcf_bpl_plan(c, m.base, m.base + beg, m.base + end);
            if (P.touched) apart = true; else bn[b] = McfBlkMeta{P.nbase, m.rrel};
        }
        if (apart) {
            const int32_t slot = atomicAdd(&s_nt, 1);
            if (slot < kBplTouchedCap) s_tb[slot] = b;   // (cannot overflow: grid sized by mcf_create)
        }
    }
    __syncthreads();
    // ---- B
    const int32_t nt = s_nt < kBplTouchedCap ? s_nt : kBplTouchedCap;
    if (nt == 0) return;   // (uniform: the usual case for every workgroup but a few)
    // the elements of T2 look their new position up in the segment table (a binary search: log2(nseg) dependent loads each):
    // from LDS when the table fits (a stem of <= 511 nodes), staged by the whole workgroup in one round trip
    McfView segv = v;
    if (c.nseg <= kBplSegLds) {
        if ((int32_t)threadIdx.x < c.nseg) s_seg[threadIdx.x] = g.seg[threadIdx.x];
        __syncthreads();
        segv.seg = s_seg;
    }
    for (int32_t t = wave; t < nt; t += kBplThreads / 64) bpl_block<MARK, RC>(v, segv, c, g.ctx, s_tb[t], lane, s_t2, &s_nn);
    if (!RC) return;
    __syncthreads();
    // ---- C
    const int32_t nn = s_nn < kBplT2Cap ? s_nn : kBplT2Cap;
    for (int32_t t = threadIdx.x >> 4; t < nn; t += kBplThreads / 16) bpl_patch_node<MARK>(v, c, s_t2[t], threadIdx.x & 15, 16);
}

// ------------------------------------------------------------------ k_reduce (multi-GPU: local best -> 16 bytes)
__global__ __launch_bounds__(kReduceThreads) void k_reduce(const McfCand* __restrict__ cand, int ncand,
                                                            McfCand* __restrict__ out) {
    int64_t key = 0, arc = -1;
    for (int i = threadIdx.x; i < ncand; i += kReduceThreads) {
        const McfCand cd = cand[i];
        if (mcf_cand_better(cd.key, cd.arc, key, arc)) { key = cd.key; arc = cd.arc; }
    }
    block_argmax<kReduceThreads>(key, arc);
    if (threadIdx.x == 0) *out = McfCand{key, arc};
}

// ------------------------------------------------------------------ k_pivot
// One workgroup; latency-bound, so the point is to keep the chain of dependent global round trips short:
// the control block is staged in LDS for the whole kernel (begin / decide / finish read and write dozens
// of its fields), the candidate loads are in flight while it arrives, the cycle comes from the
// position-space scan (~4 dependent round trips whatever its length) with the hit list in LDS.
#ifdef MCF_STAMPS
__device__ unsigned long long g_pivot_stamps[24];
#endif
constexpr int kHitsLds = 4096;  // hit-list entries kept in LDS (a longer cycle spills to global scratch)
constexpr int kSmallPath = 512;  // cycles up to this many nodes are recorded in LDS instead of the global path scratch

// LDS state of one pivoting workgroup (k_pivot, k_solve_mid)
struct PivotShared {
    McfCtx ctx;
    McfCycle cy;
    McfScanAcc acc;
    int go;  // 0 = nothing to pivot on, 1 = the climb reached the join, 2 = the scan has to finish the cycle
    // candidate cache: the winning entry (its index in the list, -1: none / not cached) and its record
    int64_t win_arc;
    int32_t win_idx;
    McfCandX winx;
    int32_t dirty_hdr[20];   // incremental sweeps: nlb, lo[8], hi[8] of McfDirty (the marking's look-ups then stay in LDS)
    McfHit hits[kHitsLds];
    int32_t path[2][kSmallPath], ppos[2][kSmallPath], pslot[2][kSmallPath];
    McfNode rec[2][kSmallPath];
    int64_t flow[2][kSmallPath];
};
static_assert(sizeof(McfCtx) % 4 == 0 && kCtxWords <= kPivotThreads, "control block staging");

// From the chosen entering arc to the updated flows / tree records / apply descriptor.  `v.ctx` must point at
// S.ctx; (key, arc) valid in thread 0; `priced` = arcs this pass evaluated (accounting).  All threads call it.
// `cached`: S.win_idx / S.winx hold the winner's candidate record (candidate cache)
template <int NT = kPivotThreads>   // NT: threads of the calling workgroup
__device__ __forceinline__ void pivot_core(const McfView& v, PivotShared& S, int64_t key, int64_t arc, int32_t rule,
                                            int64_t priced, bool cached = false) {
    const McfPaths gp = mcf_view_paths(v);                                                    // cycle scratch in global memory
    // ... and in LDS
    const McfPaths sp = McfPaths{S.path[0], S.path[1], S.rec[0], S.rec[1], S.ppos[0], S.ppos[1], S.flow[0], S.flow[1], S.pslot[0], S.pslot[1]};
    if (threadIdx.x == 0) {
        McfCtx* c = v.ctx;
        if (c->pivots < c->max_pivots) c->arcs_priced += priced;  // whole-job accounting: the arcs of this pass over ALL shards
        int go = 0;
        const bool have_wx = cached && arc >= 0 && S.win_idx >= 0;
        if (mcf_pivot_begin_t<true>(v, key, arc, rule, have_wx ? &S.winx : nullptr, &S.cy)) {   // (also what mcf_cycle_init would do)
            MCF_PSTAMP(2);
            // sequential part: at most climb_budget dependent round trips.  Shallow end points (the depth gate) are climbed
            // outright: that path is short, so it is recorded in LDS, with the arcs' flows -- decide and finish then work
            // from LDS and the flow update is store-only, as after a scan.
            const int32_t deep = S.cy.ru.depth > S.cy.rw.depth ? S.cy.ru.depth : S.cy.rw.depth;
            const bool gate = v.psz[0] && deep <= c->climb_depth && deep < kSmallPath;
            bool ok;
            if (gate) { ok = mcf_pivot_climb(v, sp, &S.cy, INT32_MAX); S.cy.small = 1; }
            else ok = mcf_pivot_climb(v, gp, &S.cy, mcf_climb_budget(v, S.cy));
            if (ok) go = S.cy.u == S.cy.w ? 1 : 2;
            if (go == 2) mcf_scan_init(&S.acc);
        }
        S.go = go;
    }
    __syncthreads();
    MCF_PSTAMP(3);
    const int go = S.go;
    if (go == 2) mcf_pivot_scan(v, sp, kSmallPath, &S.cy, &S.acc, S.hits, kHitsLds, threadIdx.x, NT);  // barriers inside
    // S.cy.small is written by lane 0 at the very end of the scan: lane 0 may use it at once, the others after the barrier.
    // Separate calls for the two scratch locations: each inlined copy works on one known address space.
    if (go && threadIdx.x == 0 && S.ctx.status == MCF_RUNNING) {
        // (two calls, one per scratch location, were merged by the compiler into one body that fetched its pointers from a
        //  table in private memory -- two dependent scratch loads on the serial path; selected here they stay in registers)
        const bool sm = S.cy.small != 0;
        const McfPaths pp = McfPaths{sm ? sp.path1 : gp.path1, sm ? sp.path2 : gp.path2, sm ? sp.rec1 : gp.rec1, sm ? sp.rec2 : gp.rec2,
                                     sm ? sp.ppos1 : gp.ppos1, sm ? sp.ppos2 : gp.ppos2, sm ? sp.flow1 : gp.flow1, sm ? sp.flow2 : gp.flow2,
                                     sm ? sp.slot1 : gp.slot1, sm ? sp.slot2 : gp.slot2};
        mcf_pivot_decide(v, pp, S.cy);
    }
    MCF_PSTAMP(8);
    __syncthreads();
    if (go && S.cy.small) mcf_pivot_finish(v, sp, threadIdx.x, NT);  // array updates, one path element per lane
    else mcf_pivot_finish(v, gp, threadIdx.x, NT);
    // candidate cache: the entering arc's entry follows its new state (basic after a swap, the other bound after a flip);
    // the leaving arc's entry, if it is listed, and every entry's reduced cost are the update pass's business
    if (cached && threadIdx.x == 0 && S.win_idx >= 0 && S.ctx.stage != 0)
        v.candx[S.win_idx].state = S.ctx.stage == 1 ? -S.ctx.pv_s : 0;
    MCF_PSTAMP(9);
}

// MARK: the handle prices incrementally, the entering / leaving arc's blocks are flagged.  BPL: the tree lives in the blocked
// preorder list (a dense-array handle's instantiation folds every branch of it away: they cost the dense path ~4 %).
// `g_list`: the handle's own candidate list -- only for it does the candidate cache hold the records
template <bool MARK, bool BPL>
__global__ __launch_bounds__(kPivotThreads) void k_pivot(McfView g, const McfCand* __restrict__ cand, int ncand,
                                                          int32_t rule, int have_sweep, const McfCand* g_list) {
    __shared__ PivotShared S;
#ifdef MCF_STAMPS
    if (threadIdx.x == 0) { for (int i = 0; i < 24; ++i) mcf_stamp_acc[i] = 0; mcf_stamp_last = __builtin_amdgcn_s_memtime(); }
#endif
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(&S.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(g.ctx)[threadIdx.x];
    // the first two candidates of every lane are in flight together with the control block (the grid leaves at most 2 048);
    // candidate cache (g.candx): the records instead -- they hold everything a minor iteration needs
    const bool cached = g.candx != nullptr && rule == MCF_RULE_CANDIDATE_LIST && ncand <= 2 * kPivotThreads && cand == g_list;
    McfCand first = McfCand{0, -1}, second = McfCand{0, -1};
    McfCandX x0, x1;
    x0.arc = -1; x1.arc = -1; x0.rc = 0; x1.rc = 0; x0.state = 0; x1.state = 0; x0.tail = x0.head = x1.tail = x1.head = 0;
    if ((int)threadIdx.x < ncand) { if (cached) x0 = g.candx[threadIdx.x]; else first = cand[threadIdx.x]; }
    if ((int)threadIdx.x + kPivotThreads < ncand) { if (cached) x1 = g.candx[threadIdx.x + kPivotThreads]; else second = cand[threadIdx.x + kPivotThreads]; }
    if (threadIdx.x == 0) S.win_idx = -1;
    if (MARK && g.dirty && threadIdx.x >= 512 && threadIdx.x < 512 + 17) S.dirty_hdr[threadIdx.x - 512] = reinterpret_cast<const int32_t*>(g.dirty)[threadIdx.x - 512];
    __syncthreads();
    McfView v = g;
    v.ctx = &S.ctx;
    if (!MARK) v.dirty = nullptr;  // folds the marking away
    else v.dirty_hdr = reinterpret_cast<const McfDirty*>(S.dirty_hdr);
    if (!BPL) { v.bmeta[0] = nullptr; v.bmeta[1] = nullptr; }  // folds the blocked list away
    MCF_PSTAMP(0);
    // candidate-list rule: slots without a pricing launch in front (have_sweep == 0) can only run
    // minor iterations; once the list is exhausted they idle until the next slot that sweeps
    if (S.ctx.status != MCF_RUNNING || (!have_sweep && S.ctx.minor_left <= 0)) {
        if (threadIdx.x == 0) g.ctx->apply = 0;
        return;
    }
    int64_t key = 0, arc = -1;
    // candidate-list rule, minor iteration: no sweep ran; the listed arcs are re-priced here
    // against the current state (resident reduced cost or potentials)
    const bool minor = rule == MCF_RULE_CANDIDATE_LIST && S.ctx.minor_left > 0;
    // accounting: arcs this pass covers over ALL shards.  Devex: the block's size comes from the host-made granule
    // totals (two loads, in flight during the arg-max)
    int64_t priced = minor ? ncand : v.m;
    if (threadIdx.x == 0 && rule == MCF_RULE_DEVEX_BLOCK && v.dx && S.ctx.num_blocks > 1)
        priced = mcf_devex_block_arcs(v.dx, (int32_t)S.ctx.block_index, S.ctx.block_granules);
    if (cached) {
        // keys straight from the records (a fresh sweep's record gives the sweep's key; an entry a clean incremental block
        // kept, or one that pivots have touched since, gives what a sweep would find now)
        const int64_t v0 = -(int64_t)x0.state * x0.rc, v1 = -(int64_t)x1.state * x1.rc;
        const int64_t k0 = (x0.arc >= 0 && v0 > 0) ? mcf_dantzig_key(v, x0.arc & 0xffffffff, v0, x0.state) : 0;
        const int64_t k1 = (x1.arc >= 0 && v1 > 0) ? mcf_dantzig_key(v, x1.arc & 0xffffffff, v1, x1.state) : 0;
        if (mcf_cand_better(k0, x0.arc, key, arc)) { key = k0; arc = x0.arc; }
        if (mcf_cand_better(k1, x1.arc, key, arc)) { key = k1; arc = x1.arc; }
    } else if (minor && v.rcache && !v.rc_partial) {
        // re-pricing from the resident reduced costs: state and reduced cost of both listed arcs of a lane are requested
        // at once, unconditionally (a dead entry reads arc 0) -- ONE round trip for the whole list instead of a chain of
        // candidate -> state -> reduced cost per entry (measured at 2 048 entries: 5.6 us of a 17 us launch)
        const int64_t e0 = first.arc < 0 ? 0 : (first.arc & 0xffffffff), e1 = second.arc < 0 ? 0 : (second.arc & 0xffffffff);
        const int32_t s0 = v.state[e0], s1 = v.state[e1];
        const int64_t r0 = v.rcache[e0], r1 = v.rcache[e1];
        const int64_t v0 = -(int64_t)s0 * r0, v1 = -(int64_t)s1 * r1;
        const int64_t k0 = (first.arc >= 0 && v0 > 0) ? mcf_dantzig_key(v, e0, v0, s0) : 0;
        const int64_t k1 = (second.arc >= 0 && v1 > 0) ? mcf_dantzig_key(v, e1, v1, s1) : 0;
        if (mcf_cand_better(k0, first.arc, key, arc)) { key = k0; arc = first.arc; }
        if (mcf_cand_better(k1, second.arc, key, arc)) { key = k1; arc = second.arc; }
        for (int i = threadIdx.x + 2 * kPivotThreads; i < ncand; i += kPivotThreads) {   // (longer gathered lists)
            const McfCand cd = cand[i];
            const int64_t kk = mcf_minor_key(v, cd.arc);
            if (mcf_cand_better(kk, cd.arc, key, arc)) { key = kk; arc = cd.arc; }
        }
    } else
    for (int i = threadIdx.x; i < ncand; i += kPivotThreads) {
        const McfCand cd = i == (int)threadIdx.x ? first : (i == (int)threadIdx.x + kPivotThreads ? second : cand[i]);
        const int64_t kk = minor ? mcf_minor_key(v, cd.arc) : cd.key;
        if (mcf_cand_better(kk, cd.arc, key, arc)) { key = kk; arc = cd.arc; }
    }
    if (ncand <= 64) {  // one wave holds every candidate: no cross-wave stage
        if (threadIdx.x < 64) wave_argmax(key, arc);
    } else {
        block_argmax<kPivotThreads>(key, arc);
    }
    if (cached) {   // who won?  its lane hands the record over (two barriers: cheaper than looking the arc up again)
        if (threadIdx.x == 0) S.win_arc = key > 0 ? arc : -1;
        __syncthreads();
        const int64_t wa = S.win_arc;
        if (wa >= 0 && x0.arc == wa) { S.winx = x0; S.win_idx = (int32_t)threadIdx.x; }
        else if (wa >= 0 && x1.arc == wa) { S.winx = x1; S.win_idx = (int32_t)threadIdx.x + kPivotThreads; }
        __syncthreads();
    }
    MCF_PSTAMP(1);
    pivot_core(v, S, key, arc, rule, priced, cached);
    // publish the control block for the apply / pricing launches that follow (finish only reads it)
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(g.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(&S.ctx)[threadIdx.x];
#ifdef MCF_STAMPS
    __syncthreads();
    MCF_PSTAMP(10);
    if (threadIdx.x == 0) { for (int i = 0; i < 24; ++i) g_pivot_stamps[i] += mcf_stamp_acc[i]; g_pivot_stamps[23] += 1; }
#endif
}

// ------------------------------------------------------------------ k_pivot_run: pivots of a candidate list back to back
// Blocked list + candidate cache + candidate-list rule.  Almost every pivot of a large sparse instance re-hangs a handful of
// nodes: its whole update is a few block records, a few dozen reduced costs and the list's records -- work for ONE workgroup.
// This kernel therefore keeps going: pivot, update in place (bpl_update_inline), next minor iteration, ... until the list is
// used up, a pivot's update is too large for one workgroup (the descriptor is then left for the k_update_bpl launch that
// follows, exactly as k_pivot leaves it) or `max_steps` is reached.  What it saves per pivot: two launch boundaries, the
// control block's trip through memory and back, the staging of the list.  The pivots are the same ones in the same order:
// every step is k_pivot's step and k_update_bpl's passes, run by one workgroup instead of a grid.
constexpr int kRunTouchedCap = 2048, kRunT2Cap = 2048, kRunSegCap = 256;
constexpr int kRunMaxSubtree = 64;     // larger re-hung subtrees go to the grid

struct RunShared {
    int32_t nt, nn;
    int32_t tb[kRunTouchedCap];
    int32_t t2[kRunT2Cap];
    McfSeg seg[kRunSegCap];
};

// k_update_bpl's passes by the calling workgroup alone (NT threads; not for ctx.rebuild).  `c` is the control block in LDS.
template <bool MARK, bool RC, int NT>
__device__ __forceinline__ void bpl_update_inline(const McfView& v, McfCtx& c, RunShared& R) {
    const int32_t tid = (int32_t)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) { R.nt = 0; R.nn = 0; }
    if (tid < c.nseg && tid < kRunSegCap) R.seg[tid] = v.seg[tid];
    __syncthreads();
    McfView segv = v;
    if (c.nseg <= kRunSegCap) segv.seg = R.seg;
    const int32_t known0 = c.t2_blk, known1 = c.ins_blk;
    const bool preview = RC && c.pv_t2n == 1;
    const McfBlkMeta* bm = c.cur ? v.bmeta[1] : v.bmeta[0];
    McfBlkMeta* bn = c.cur ? v.bmeta[0] : v.bmeta[1];
    const int32_t* xa = c.arena ? v.bext[1] : v.bext[0];
    if (wave < 2) {
        const int32_t kb = wave == 0 ? known0 : ((known1 >= 0 && known1 != known0) ? known1 : -1);
        if (kb >= 0) bpl_block<MARK, RC>(v, segv, c, &c, kb, lane, R.t2, &R.nn, !preview, kRunT2Cap);
    } else if (preview && wave >= NT / 128) {
        // the one node of T2: its adjacency range came with the pivot (second half of the workgroup)
        const int64_t sigma = c.sigma;
        const int32_t t0 = tid - NT / 2, nt = NT / 2;
        for (int64_t p = c.pv_adj[0] + t0; p < c.pv_adj[1]; p += nt) {
            const int64_t ent = v.adj[p];
            const int32_t e = (int32_t)((uint32_t)ent >> 1);
            const int64_t r = v.rcache[e] + ((ent & 1) ? sigma : -sigma);
            v.rcache[e] = r;
            if (v.vkey) v.vkey[e] = mcf_vkey(-(int64_t)v.state[e] * r, v.vk_bigm, v.vk_half);
            if (MARK) mcf_mark_dirty(v, e);
        }
    } else {
        // phase A: the other blocks, one lane per block (the lanes of waves 2 .. that are not patching)
        const int32_t a_lanes = (preview ? NT / 2 : NT) - 128, a0 = tid - 128;
        const int32_t nold = c.alloc_prev;
        // eight blocks per lane and trip, all their loads in flight together (one block per trip was a chain of dependent
        // round trips: 20 K blocks over 400-900 lanes = 25-50 of them per pivot)
        constexpr int KA = 8;
        for (int32_t b0 = a0; b0 < nold; b0 += a_lanes * KA) {
            McfBlkMeta mm[KA];
            int32_t xx[KA];
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                const int32_t b = b0 + k * a_lanes;
                const int32_t bc = b < nold ? b : a0;   // clamp: keep the loads unconditional
                mm[k] = bm[bc];
                xx[k] = xa[bc];
            }
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                const int32_t b = b0 + k * a_lanes;
                if (b >= nold || b == known0 || b == known1) continue;
                const McfBlkMeta m = mm[k];
                const int32_t x = xx[k], beg = mcf_ext_beg(x), end = mcf_ext_end(x);
                if (m.base == MCF_BLK_FREE || end <= beg) { bn[b] = McfBlkMeta{MCF_BLK_FREE, 0}; continue; }
                bool apart = (x & MCF_EXT_FLAG) != 0;
                if (!apart) {
                    const McfBlkPlan P = mcf_bpl_plan(c, m.base, m.base + beg, m.base + end);
                    if (P.touched) apart = true; else bn[b] = McfBlkMeta{P.nbase, m.rrel};
                }
                if (apart) {
                    const int32_t slot = atomicAdd(&R.nt, 1);
                    if (slot < kRunTouchedCap) R.tb[slot] = b;
                }
            }
        }
    }
    __syncthreads();
    const int32_t nt = R.nt < kRunTouchedCap ? R.nt : kRunTouchedCap;   // (at most the re-index flags of the cycle + T2's other blocks)
    for (int32_t t = wave; t < nt; t += NT / 64) bpl_block<MARK, RC>(v, segv, c, &c, R.tb[t], lane, R.t2, &R.nn, !preview, kRunT2Cap);
    __syncthreads();
    if (RC && !preview) {
        const int32_t nn = R.nn < kRunT2Cap ? R.nn : kRunT2Cap;
        const bool whole = nn == c.t2_size && nn <= kBplListMember;
        for (int32_t t = tid >> 4; t < nn; t += NT / 16) bpl_patch_node<MARK>(v, c, R.t2[t], tid & 15, 16, whole ? R.t2 : nullptr, nn);
    }
    candx_pass(v, c, tid, NT);
}

template <bool MARK, bool RC>
__global__ __launch_bounds__(kPivotThreads) void k_pivot_run(McfView g, int ncand, int have_sweep, int max_steps) {
    __shared__ PivotShared S;
    __shared__ RunShared R;
#ifdef MCF_STAMPS
    if (threadIdx.x == 0) { for (int i = 0; i < 24; ++i) mcf_stamp_acc[i] = 0; mcf_stamp_last = __builtin_amdgcn_s_memtime(); }
#endif
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(&S.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(g.ctx)[threadIdx.x];
    if (MARK && g.dirty && threadIdx.x >= 512 && threadIdx.x < 512 + 17) S.dirty_hdr[threadIdx.x - 512] = reinterpret_cast<const int32_t*>(g.dirty)[threadIdx.x - 512];
    __syncthreads();
    McfView v = g;
    v.ctx = &S.ctx;
    if (!MARK) v.dirty = nullptr;
    else v.dirty_hdr = reinterpret_cast<const McfDirty*>(S.dirty_hdr);
    if (threadIdx.x == 0) S.ctx.apply = 0;   // (a descriptor left by an earlier launch has been carried out by the update launch in between)
    const int32_t rule = MCF_RULE_CANDIDATE_LIST;
    int steps = 0;
    for (;; ++steps) {
        // uniform control values are read BEFORE a barrier (lane 0 rewrites them later in the iteration)
        const int32_t status_now = S.ctx.status, minor_left = S.ctx.minor_left;
        const bool sweep_now = steps == 0 && have_sweep;
        __syncthreads();
        if (steps >= max_steps || status_now != MCF_RUNNING || (!sweep_now && minor_left <= 0)) break;
        MCF_PSTAMP(0);
        // the list's records (kept current by the update passes; after this workgroup's own in-place updates they come from its
        // L2): state and exact reduced cost give the key a sweep would find now
        McfCandX x0, x1;
        x0.arc = -1; x1.arc = -1; x0.rc = 0; x1.rc = 0; x0.state = 0; x1.state = 0; x0.tail = x0.head = x1.tail = x1.head = 0;
        if ((int)threadIdx.x < ncand) x0 = g.candx[threadIdx.x];
        if ((int)threadIdx.x + kPivotThreads < ncand) x1 = g.candx[threadIdx.x + kPivotThreads];
        if (threadIdx.x == 0) S.win_idx = -1;
        int64_t key = 0, arc = -1;
        const int64_t v0 = -(int64_t)x0.state * x0.rc, v1 = -(int64_t)x1.state * x1.rc;
        const int64_t k0 = (x0.arc >= 0 && v0 > 0) ? mcf_dantzig_key(v, x0.arc & 0xffffffff, v0, x0.state) : 0;
        const int64_t k1 = (x1.arc >= 0 && v1 > 0) ? mcf_dantzig_key(v, x1.arc & 0xffffffff, v1, x1.state) : 0;
        if (mcf_cand_better(k0, x0.arc, key, arc)) { key = k0; arc = x0.arc; }
        if (mcf_cand_better(k1, x1.arc, key, arc)) { key = k1; arc = x1.arc; }
        const int64_t priced = minor_left > 0 ? ncand : v.m;
        if (ncand <= 64) { if (threadIdx.x < 64) wave_argmax(key, arc); }
        else block_argmax<kPivotThreads>(key, arc);
        if (threadIdx.x == 0) S.win_arc = key > 0 ? arc : -1;
        __syncthreads();
        const int64_t wa = S.win_arc;
        if (wa >= 0 && x0.arc == wa) { S.winx = x0; S.win_idx = (int32_t)threadIdx.x; }
        else if (wa >= 0 && x1.arc == wa) { S.winx = x1; S.win_idx = (int32_t)threadIdx.x + kPivotThreads; }
        __syncthreads();
        MCF_PSTAMP(1);
        pivot_core(v, S, key, arc, rule, priced, true);
        __syncthreads();
        if (!S.ctx.apply) continue;   // a bound flip (or nothing to pivot on): no tree change
        // the update: here when it is small, else by the grid launch that follows
        if (S.ctx.rebuild || S.ctx.t2_size > kRunMaxSubtree) break;
        bpl_update_inline<MARK, RC, kPivotThreads>(v, S.ctx, R);
        __syncthreads();
        if (threadIdx.x == 0) S.ctx.apply = 0;   // (pending_flip stays: the next begin switches to the copies just written)
        // what this workgroup has just stored must not be served from a stale line of the scalar cache (uniform loads of the
        // block records); the vector L1 is write-through and shared by the whole workgroup
        __builtin_amdgcn_s_dcache_inv();
    }
    __syncthreads();
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(g.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(&S.ctx)[threadIdx.x];
#ifdef MCF_STAMPS
    __syncthreads();
    MCF_PSTAMP(10);
    if (threadIdx.x == 0) { for (int i = 0; i < 24; ++i) g_pivot_stamps[i] += mcf_stamp_acc[i]; g_pivot_stamps[23] += steps; }
#endif
}

// ------------------------------------------------------------------ k_solve_mid: persistent single-workgroup pivot loop, state in global memory
// Between two kernels of the three-kernel path every first touch of the tree arrays is a miss to the memory-side
// cache (the previous kernel wrote them from other CUs / XCDs): ~0.7 us per dependent round trip, ~12 of them in
// k_pivot alone.  For mid-size instances one workgroup can do the WHOLE pivot -- pricing of a Devex block (or, for
// the candidate-list rule, re-pricing the list), cycle scan, finish, block permutation + potential shift, resident
// reduced-cost update -- and then nothing crosses a kernel boundary: the state stays in this CU's L1 / this XCD's
// L2 for as many pivots as the rule allows.  Same core functions, same arc sets and tie rules as the other paths,
// hence the identical pivot sequence.
//   Devex block / small Dantzig:  one launch runs until optimal / pivot limit.
//   candidate list:               the launch ends when a full sweep is due (k_price_rc over the whole grid builds
//                                 the next list); `fresh` says such a sweep ran right before this launch.

// `arm`: take the pivot cap from the kernel argument (what k_ctl does for the other paths: one launch less per call;
// only for launches that are not replayed from a captured graph, whose arguments are frozen).
__device__ __forceinline__ void arm_ctx(McfCtx* c, int64_t cap) {
    c->max_pivots = cap;
    c->limit_checked = 0;
    if (c->status == MCF_PIVOT_LIMIT && c->pivots < cap) c->status = MCF_RUNNING;
}

// Devex: the granule range [bg0, bg1) of the current block; every other rule: all granules
__device__ __forceinline__ void devex_block_granules(const McfCtx& c, bool devex, int32_t& bg0, int32_t& bg1) {
    int32_t lo = 0, hi = MCF_GRANULES;
    if (devex) {
        const int32_t bg = c.block_granules;
        lo = (int32_t)c.block_index * bg;
        if (lo >= MCF_GRANULES) lo = 0;
        hi = lo + bg < MCF_GRANULES ? lo + bg : MCF_GRANULES;
    }
    bg0 = lo; bg1 = hi;
}

// The candidate-list rule's full sweep done by ONE workgroup (batched persistent loops: no grid to go back to): wave w
// plays the pricing workgroups w, w + nwaves, ... of the grid sweep -- the same arc sets (workgroup lb * 8 + x: the groups of
// four arcs g_lo(x) + lb * 256 + [0, 256) + j * nlb * 256 of bucket x, as in k_price_rc / mcf_price_block_of), the same keys,
// the same tie rule -- and writes the same list, one candidate per (virtual) workgroup.
template <int NT>
__device__ __forceinline__ void virtual_list_sweep(const McfView& v, McfCand* list, int nlist) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nlb = nlist / MCF_NUM_BUCKETS;
    const int8_t* __restrict__ state = v.state;
    const int64_t* __restrict__ rcache = v.rcache;
    const int32_t* __restrict__ orig = v.orig;
    for (int b = wave; b < nlist; b += NT / 64) {
        const int x = b & (MCF_NUM_BUCKETS - 1), lb = b >> 3;
        const int64_t lo = v.bucket_off[x], hi = v.bucket_off[x + 1];
        const int64_t g_lo = lo >> 2, g_hi = (hi + 3) >> 2;
        int64_t key = 0, best_i = -1;
        for (int64_t gbase = g_lo + (int64_t)lb * 256; gbase < g_hi; gbase += (int64_t)nlb * 256) {
            for (int t = lane; t < 256; t += 64) {
                const int64_t g = gbase + t;
                if (g >= g_hi) break;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t i = (g << 2) + k;
                    if (i < lo || i >= hi) continue;
                    const int32_t s = state[i];
                    if (s == 0) continue;
                    const int64_t viol = -(int64_t)s * rcache[i];
                    if (viol <= 0) continue;
                    const int64_t kk = mcf_dantzig_key(v, i, viol, s);
                    if (kk < key) continue;
                    if (kk > key || best_i < 0 || orig[i] < orig[best_i]) { key = kk; best_i = i; }
                }
            }
        }
        int64_t arc = best_i >= 0 ? mcf_pack_arc(orig[best_i], best_i) : -1;
        wave_argmax(key, arc);
        if (lane == 0) list[b] = McfCand{key, arc};
    }
}

// NT: threads of the workgroup (the batched launch also runs narrower workgroups, two per CU).  SELF: a candidate-list loop does
// the list's full sweeps itself (cand is then written as well as read).  A template parameter, not a run-time flag: with the
// sweep inlined into every instance the loop's register demand went up (spills 9 -> 21 VGPRs, scratch 72 -> 488 B) and
// every rule lost 30-45 % -- only the kernels that need it carry it.
template <int NT = kPivotThreads, bool SELF = false>
__device__ __forceinline__ void solve_mid_body(const McfView& g, int32_t rule, McfCand* cand,
                                               int ncand, int fresh, int max_iters, int arm, int64_t cap, McfCtx* host_ctx = nullptr) {
    __shared__ PivotShared S;
    __shared__ int32_t s_gran[MCF_NUM_BUCKETS][MCF_GRANULES + 1];  // Devex: the granule table (blocks move and resize under the tuner)
    __shared__ int32_t s_lo[MCF_NUM_BUCKETS], s_hi[MCF_NUM_BUCKETS];  // other rules: the whole buckets
#ifdef MCF_STAMPS
    if (threadIdx.x == 0) { for (int i = 0; i < 24; ++i) mcf_stamp_acc[i] = 0; mcf_stamp_last = __builtin_amdgcn_s_memtime(); }
    __syncthreads();
#endif
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(&S.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(g.ctx)[threadIdx.x];
    const bool devex = rule == MCF_RULE_DEVEX_BLOCK && g.dx;
    if (devex) {
        for (int q = threadIdx.x; q < MCF_NUM_BUCKETS * (MCF_GRANULES + 1); q += NT)
            (&s_gran[0][0])[q] = (&g.dx->gran[0][0])[q];
    } else if (threadIdx.x < MCF_NUM_BUCKETS) {
        s_lo[threadIdx.x] = (int32_t)g.bucket_off[threadIdx.x];
        s_hi[threadIdx.x] = (int32_t)g.bucket_off[threadIdx.x + 1];
    }
    __syncthreads();
    if (arm && threadIdx.x == 0) arm_ctx(&S.ctx, cap);
    __syncthreads();
    McfView v = g;
    v.ctx = &S.ctx;
    v.dirty = nullptr;  // mcf_create never combines incremental sweeps with this loop: the marking folds away
    v.dirty_hdr = nullptr; v.bmeta[0] = nullptr; v.bmeta[1] = nullptr; v.candx = nullptr;   // (nor the blocked list, nor the candidate cache)
    const bool listing = rule == MCF_RULE_CANDIDATE_LIST;
    // the sweep in front of this launch was a no-op if the list was still live (k_price_rc, use_block == 2)
    bool have_fresh = listing && fresh && S.ctx.minor_left <= 0 && S.ctx.status == MCF_RUNNING;
    for (int it = 0; it < max_iters; ++it) {
        // uniform control values are read BEFORE a barrier: lane 0 rewrites them later in this very iteration
        const int32_t status_now = S.ctx.status;
        const int32_t minor_left = S.ctx.minor_left;
        int32_t bg0, bg1;
        devex_block_granules(S.ctx, devex, bg0, bg1);
        __syncthreads();
        if (status_now != MCF_RUNNING) break;
        MCF_PSTAMP(0);
        int64_t key = 0, arc = -1, priced = 0;
        if (listing) {
            const bool minor = minor_left > 0;
            if (!minor && !have_fresh) {
                if constexpr (!SELF) break;  // a full sweep is due: back to the grid
                else {
                    virtual_list_sweep<NT>(v, cand, ncand);
                    __syncthreads();         // the list (global memory, this workgroup's own writes) before anyone reads it
                }
            }
            have_fresh = false;
            for (int i = threadIdx.x; i < ncand; i += NT) {
                const McfCand cd = cand[i];
                const int64_t kk = minor ? mcf_minor_key(v, cd.arc) : cd.key;
                if (mcf_cand_better(kk, cd.arc, key, arc)) { key = kk; arc = cd.arc; }
            }
            priced = minor ? ncand : v.m;
            if (ncand <= 64) { if (threadIdx.x < 64) wave_argmax(key, arc); }
            else block_argmax<NT>(key, arc);
        } else {
            // the arc set of k_price_rc for shard 0 of 1: 128 lanes per head bucket, all eight buckets at once,
            // streaming the resident reduced costs
            constexpr int kPer = NT / MCF_NUM_BUCKETS;
            const int x = threadIdx.x / kPer, l = threadIdx.x % kPer;
            const int64_t lo = devex ? s_gran[x][bg0] : s_lo[x], hi = devex ? s_gran[x][bg1] : s_hi[x];
            const int64_t* __restrict__ rcache = v.rcache;
            const int8_t* __restrict__ state = v.state;
            int64_t best_i = -1;  // the caller's id is looked up once at the end (and on ties)
            int32_t best_s = 0;
            constexpr int UM = 4;  // arcs in flight per lane: all loads first (unconditional, clamped), then the arithmetic
            if (hi - lo <= kPer) {  // at most one arc per lane (small Devex blocks): nothing to overlap
                const int64_t i = lo + l;
                if (i < hi && state[i]) {
                    const int64_t viol = -(int64_t)state[i] * rcache[i];
                    if (viol > 0) {
                        key = mcf_dantzig_key(v, i, viol, (int32_t)state[i]);
                        if (rule == MCF_RULE_DEVEX_BLOCK) key = __double_as_longlong(((double)viol * (double)viol) / (double)v.weight[i]);
                        best_i = i;
                        best_s = state[i];
                    }
                }
            } else
            for (int64_t i0 = lo + l; i0 < hi; i0 += (int64_t)kPer * UM) {
                int32_t sts[UM];
                int64_t rcs[UM];
                float wts[UM];
#pragma unroll
                for (int u = 0; u < UM; ++u) {
                    const int64_t i = i0 + (int64_t)u * kPer;
                    const int64_t ic = i < hi ? i : lo;
                    sts[u] = i < hi ? (int32_t)state[ic] : 0;
                    rcs[u] = rcache[ic];
                    wts[u] = rule == MCF_RULE_DEVEX_BLOCK ? v.weight[ic] : 1.0f;
                }
#pragma unroll
                for (int u = 0; u < UM; ++u) {
                    const int64_t i = i0 + (int64_t)u * kPer;
                    if (!sts[u]) continue;
                    const int64_t viol = -(int64_t)sts[u] * rcs[u];
                    if (viol <= 0) continue;
                    int64_t kk = mcf_dantzig_key(v, i, viol, sts[u]);
                    if (rule == MCF_RULE_DEVEX_BLOCK) {
                        const double merit = ((double)viol * (double)viol) / (double)wts[u];
                        kk = __double_as_longlong(merit);
                    }
                    if (kk < key) continue;
                    if (kk > key) { key = kk; best_i = i; best_s = sts[u]; }
                    else if (best_i < 0) { best_i = i; best_s = sts[u]; }
                    else {
                        const int32_t a = devex ? mcf_devex_tie_id(v.orig[i], sts[u]) : v.orig[i];
                        const int32_t b = devex ? mcf_devex_tie_id(v.orig[best_i], best_s) : v.orig[best_i];
                        if (a < b) { best_i = i; best_s = sts[u]; }
                    }
                }
            }
            if (best_i >= 0) arc = mcf_pack_arc(devex ? mcf_devex_tie_id(v.orig[best_i], best_s) : v.orig[best_i], best_i);
            if (threadIdx.x == 0)
                for (int x2 = 0; x2 < MCF_NUM_BUCKETS; ++x2) priced += devex ? s_gran[x2][bg1] - s_gran[x2][bg0] : s_hi[x2] - s_lo[x2];
            block_argmax<NT>(key, arc);
        }
        MCF_PSTAMP(1);
        pivot_core<NT>(v, S, key, arc, rule, priced);
        __syncthreads();  // the finish pass's writes (records, sizes, segment table) before the apply pass reads them
        if (S.ctx.apply) {  // (splitting the lanes between the two halves was measured and lost at 4 096 nodes)
            apply_pass(v, S.ctx, threadIdx.x, NT);
            rcupd_pass(v, S.ctx, threadIdx.x >> 4, NT / 16, threadIdx.x & 15);
        }
        __syncthreads();
        MCF_PSTAMP(10);
#ifdef MCF_STAMPS
        if (threadIdx.x == 0) mcf_stamp_acc[23] += 1;
#endif
        if (threadIdx.x == 0) S.ctx.apply = 0;
    }
    __syncthreads();
    // at the budget: is any arc still eligible?  (simplex.py:1678-1699; saves the host a pricing pass + three syncs)
    if (S.ctx.status == MCF_PIVOT_LIMIT && !S.ctx.limit_checked) {
        __shared__ int s_any;
        if (threadIdx.x == 0) s_any = 0;
        __syncthreads();
        int any = 0;
        for (int64_t i = threadIdx.x; i < g.m && !any; i += NT) {
            const int64_t st = g.state[i];
            if (st != 0 && -st * g.rcache[i] > 0) any = 1;
        }
        if (any) s_any = 1;
        __syncthreads();
        if (threadIdx.x == 0) { if (s_any) S.ctx.limit_checked = 1; else S.ctx.status = MCF_OPTIMAL; }
        __syncthreads();
    }
    if (threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(g.ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(&S.ctx)[threadIdx.x];
    if (host_ctx && threadIdx.x < kCtxWords) reinterpret_cast<int32_t*>(host_ctx)[threadIdx.x] = reinterpret_cast<const int32_t*>(&S.ctx)[threadIdx.x];
#ifdef MCF_STAMPS
    if (threadIdx.x == 0) for (int i = 0; i < 24; ++i) g_pivot_stamps[i] += mcf_stamp_acc[i];
#endif
}

__global__ __launch_bounds__(kPivotThreads) void k_solve_mid(McfView g, int32_t rule, McfCand* cand, int ncand, int fresh,
                                                              int max_iters, int arm, int64_t cap) {
    solve_mid_body(g, rule, cand, ncand, fresh, max_iters, arm, cap);
}

// Many independent instances side by side, state in global memory: workgroup b runs the whole solve of jobs[b]
// (Dantzig / Devex handles of the persistent loop; mcf_solve_batch).
struct MidJob {
    McfView g;
    int32_t rule;
    int32_t nlist;     // candidate list: its length (= the grid's pricing workgroups) ...
    McfCand* list;     // ... and where it lives
    int64_t cap;
    McfCtx* host_ctx;  // pinned: the final control block goes straight to the host
};

// 4 waves per SIMD (<= 128 VGPRs): one workgroup of 1 024 or TWO of 512 per CU -- the loop is a chain of dependent memory
// round trips, so a second instance on the CU fills the first one's waiting time (scripts/batch_mid.py, MCF_BATCH_THREADS).
template <int NT, bool SELF>   // SELF: the candidate-list jobs of a batch (their own launch)
__global__ __launch_bounds__(NT, 4) void k_solve_mid_batch(const MidJob* __restrict__ jobs) {
    const MidJob& J = jobs[blockIdx.x];   // uniform per workgroup: scalar loads
    solve_mid_body<NT, SELF>(J.g, J.rule, J.list, J.nlist, 0, 1 << 22, 1, J.cap, J.host_ctx);
}

// The reduced-cost half alone (overlapped graphs: the next pivot's pricing waits for this half only, see build_graph)
template <bool MARK>
__global__ __launch_bounds__(kRcupdThreads) void k_rcupd(McfView g) {
    McfView v = g;
    if (!MARK) v.dirty = nullptr;
    const McfCtx c = *v.ctx;
    if (!c.apply) return;
    rcupd_pass(v, c, (int64_t)blockIdx.x * (kRcupdThreads / 16) + (threadIdx.x >> 4), (int64_t)gridDim.x * (kRcupdThreads / 16), threadIdx.x & 15);
}

// ------------------------------------------------------------------ k_apply
__global__ __launch_bounds__(kApplyThreads) void k_apply(McfView v) {
    const McfCtx c = *v.ctx;  // uniform: scalar loads
    if (!c.apply) return;
    const int xb = v.candx ? kCandxBlocks : 0;   // (kApplyThreads == kRcupdThreads)
    const int nb = (int)gridDim.x - xb;
    if ((int)blockIdx.x >= nb) { candx_pass(v, c, ((int)blockIdx.x - nb) * kApplyThreads + (int)threadIdx.x, xb * kApplyThreads); return; }
    apply_pass(v, c, (int64_t)blockIdx.x * kApplyThreads + threadIdx.x, (int64_t)nb * kApplyThreads);
}

// ------------------------------------------------------------------ two-lane cycle climb (LDS loop)
// With the tree in LDS the climb is bound by instruction issue of ONE lane (~150 instructions per round trip for
// the two sides), not by latency.  Lanes 0 and 1 of a wave therefore climb one side each in lock step -- the same
// instruction stream serves both sides -- and swap (node, depth) with one DPP move per word and round trip.  The
// steps, the recorded paths and the ratio-test winners are exactly those of mcf_pivot_climb (depth-balanced: a side
// moves when it is at least as deep as the other); lane 0 gets the finished McfCycle.  Called by lanes 0 and 1 only.
__device__ __forceinline__ int swap01(int x) { return __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false); }  // quad_perm [1,0,3,2]

__device__ __forceinline__ bool pivot_climb_2lanes(const McfView& v, McfCycle* out) {
    const McfCtx* c = v.ctx;
    const int side = threadIdx.x & 1;  // 0: first side, 1: second side
    const int32_t* pcur = c->cur ? v.posbuf[1] : v.posbuf[0];
    int32_t node = side ? c->pv_second : c->pv_first;
    McfNode rec = v.node[node];
    int32_t pos = pcur[node];
    const McfNode rec0 = rec;
    const int32_t pos0 = pos;
    int32_t* const path = side ? v.path2 : v.path1;
    int32_t* const ppos = side ? v.ppos2 : v.ppos1;
    McfNode* const recs = side ? v.rec2 : v.rec1;
    int64_t d = MCF_INF;
    int32_t k = -1, n = 0, trips = 0;
    bool ok = true;
    for (;;) {
        const int32_t onode = swap01(node), odepth = swap01(rec.depth);
        if (node == onode) break;
        if (rec.depth >= odepth) {
            const McfNode nrec = v.node[rec.parent];
            const int32_t npos = pcur[rec.parent];
            const McfArcW a = v.arcw[rec.pred >> 1];
            // first side is walked against the flow (an up arc loses flow), second side with it
            const bool loses = ((rec.pred & 1) != 0) != (side != 0);
            const int64_t r = loses ? a.flow : (a.cap >= MCF_INF ? MCF_INF : a.cap - a.flow);
            if (side ? r <= d : r < d) { d = r; k = n; }
            path[n] = node;
            recs[n] = rec;
            ppos[n] = pos;
            ++n;
            node = rec.parent;
            rec = nrec;
            pos = npos;
        }
        if (++trips > v.n_nodes) { ok = false; break; }  // depths out of sync: never spin (both lanes count alike)
    }
    // hand the second side to lane 0
    const int32_t od_lo = swap01((int)(uint32_t)d), od_hi = swap01((int)(uint32_t)((uint64_t)d >> 32));
    const int32_t ok2 = swap01(k), on2 = swap01(n), opos0 = swap01(pos0);
    McfNode orec0;
    orec0.parent = swap01(rec0.parent); orec0.pred = swap01(rec0.pred); orec0.size = swap01(rec0.size); orec0.depth = swap01(rec0.depth);
    if (side == 0) {
        out->d1 = d; out->k1 = k; out->n1 = n;
        out->d2 = (int64_t)(((uint64_t)(uint32_t)od_hi << 32) | (uint32_t)od_lo); out->k2 = ok2; out->n2 = on2;
        out->u = node; out->w = node; out->pu = pos; out->pw = pos; out->ru = rec; out->rw = rec;
        out->p0u = pos0; out->p0w = opos0; out->r0u = rec0; out->r0w = orec0;
        out->small = 0;
    }
    return ok;
}

// ------------------------------------------------------------------ k_solve_small: fused LDS-resident pivot loop
// Instances whose whole state fits in one CU's 160 KiB of LDS (netgen_8_08a: ~96 KiB) are
// latency-bound, not bandwidth-bound: 27 KB per sweep is nothing, three kernel boundaries and
// a dozen dependent global loads per pivot are everything.  This kernel copies the instance
// into LDS once, runs pivots back to back in ONE persistent workgroup (price: all lanes, THREADS / 8
// per head bucket, states and potentials from LDS, the arcs' end points, costs and ids from registers;
// pivot: the same mcf_pivot_begin / mcf_pivot_decide / mcf_pivot_finish; apply: all lanes through the
// same mcf_apply_one) and copies the state back.  Same arc sets, same tie rule, same core functions
// as the three-kernel path, so the pivot sequence is identical -- at every width: the workgroup is
// THREADS lanes wide: 256, one wave per SIMD, or 1 024 when forced (small_threads_for; MCF_SMALL_THREADS).
typedef McfSmallLayout SmallLayout;   // (mcf_core.h, beside mcf_small_plan: the CPU tests plan with the same function)

constexpr int kSmallMaxLds = MCF_SMALL_MAX_LDS;   // dynamic LDS of the fused small-instance loop (160 KB per CU, under 4 KB static on top)
constexpr int kSmallCycleMaxNodes = MCF_SMALL_CYCLE_MAX_NODES;  // node-parallel cycle search up to this many tree nodes (strided over the lanes)

// Arcs of a head bucket that one lane keeps in registers (tail, head, cost, orig: 4 VGPRs each).  THREADS / 8 lanes share a
// bucket, so 320 (256 lanes) / 384 (1 024 lanes) arcs per bucket are register-resident -- netgen_8_08a's buckets hold
// 256 +- 20 -- and the rest of a fuller bucket is priced from LDS.
constexpr int small_reg_arcs(int threads) { return threads == 256 ? 10 : 3; }
// Where every wave keeps its copy of the control block: one wave per SIMD (256 lanes) has 512 vector registers to itself and
// leaves the control block where the compiler puts it; forced into the ~100 scalar registers, control block, pivot
// descriptor and the view's pointers do not fit, and their spills (v_writelane / v_readlane inside the loop) cost more than
// the mailbox did: 5.60 us per pivot against 4.80, the parent's 5.60.  Four waves per SIMD (1 024 lanes) have
// 128 vector registers each, nearly all in use: there the control block goes to scalar registers, or it would spill to
// scratch memory.
constexpr bool small_scalar_control(int threads) { return threads > 256; }
// Dantzig with the plain sweep deals the arcs evenly, not per head bucket (mcf_core.h: mcf_even_arc): lane t prices the engine
// arcs bucket_off[0] + t + slot * THREADS.  netgen_8_08a's buckets hold 229 .. 299 arcs -- 8 .. 10 slots of 32 lanes, so every
// wave ran all ten unrolled slots -- where 2 048 arcs over 256 lanes are 8.  The front kernels' loop is compiled for two slot
// counts, small_reg_arcs and small_reg_arcs_few (2 048 arcs' worth), and the launch's constant arc count picks one
// (mcf_even_reg_slots: a uniform branch).  In the front kernels only, where the deal is a compile-time constant: in the general
// kernels -- Dantzig with 64-bit keys beside Devex and the candidate list, which keeps the deal per bucket since its list is each
// bucket's best -- the stride becomes a run-time value, and Devex and the candidate list, which never deal evenly, measured
// 1.5 - 3 % slower over whole solves with it (profiles/small_loop_regs_whole_solves.txt); they keep the deal per
// bucket and the one sweep of small_reg_arcs slots.
constexpr int small_reg_arcs_few(int threads, bool front) { return !front ? small_reg_arcs(threads) : (threads == 256 ? 8 : 2); }
template <int N> struct SmallSlots { static constexpr int value = N; };

template <int THREADS>
__device__ __forceinline__ void copy_words(void* dst, const void* src, uint32_t bytes) {
    const uint32_t n = bytes >> 2;
    const int32_t* s = static_cast<const int32_t*>(src);
    int32_t* d = static_cast<int32_t*>(dst);
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) d[i] = s[i];
}

#ifdef MCF_STAMPS
#define STAMP(slot)                                                                       \
    do {                                                                                  \
        if (threadIdx.x == 0) {                                                           \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();                 \
            stamps_[slot] += now_ - last_;                                                \
            last_ = now_;                                                                 \
        }                                                                                 \
    } while (0)
#else
#define STAMP(slot) do {} while (0)
#endif
// (diagnostic build: the finishing wave's own clock -- the cycles of its finish pass, summed into slot 7 -- since lane 0's
//  stamps merge finish and apply into one figure once the two run side by side)
#ifdef MCF_STAMPS
#define MCF_LAST_WAVE_BEGIN() const unsigned long long lw0_ = __builtin_amdgcn_s_memtime()
#define MCF_LAST_WAVE_STAMP() do { last_wave_ += __builtin_amdgcn_s_memtime() - lw0_; } while (0)
#else
#define MCF_LAST_WAVE_BEGIN() do {} while (0)
#define MCF_LAST_WAVE_STAMP() do {} while (0)
#endif
// (diagnostic build, -DMCF_SLOT_PROBE=N [-DMCF_SLOT_PROBE_KIND=K]: N further independent instructions behind the arg-max of every
//  iteration, in every wave -- K = 0: s_nop 0; 1: a v_mov into a register nobody reads; 2: an s_mov likewise.  The time a pivot
//  gains per added instruction is what an issue slot of that kind costs a wave of this loop: profiles/small_loop_slots_probe.txt.
//  Never in the shipped library.)
#if defined(MCF_SLOT_PROBE) && MCF_SLOT_PROBE > 0
#ifndef MCF_SLOT_PROBE_KIND
#define MCF_SLOT_PROBE_KIND 0
#endif
__device__ __forceinline__ void mcf_slot_probe() {
#pragma unroll
    for (int i = 0; i < MCF_SLOT_PROBE; ++i) {
        if (MCF_SLOT_PROBE_KIND == 0) {
            asm volatile("s_nop 0");
        } else if (MCF_SLOT_PROBE_KIND == 1) {
            int32_t dead;
            asm volatile("v_mov_b32 %0, 0" : "=v"(dead));
            asm volatile("" ::"v"(dead));
        } else {
            int32_t dead;
            asm volatile("s_mov_b32 %0, 0" : "=s"(dead));
            asm volatile("" ::"s"(dead));
        }
    }
}
#define MCF_SLOT_PROBE_HERE() mcf_slot_probe()
#else
#define MCF_SLOT_PROBE_HERE() do {} while (0)
#endif
// (diagnostic build: EVERY wave's own clock, from the top of the iteration to where it stands -- slot 0: at the search barrier,
//  1: behind the ratio tests, 2: behind decide, 3: behind apply (its arrival at the end barrier), 4: behind finish (last wave) --
//  summed over the pivots that swap or flip; slot 5 (wave 0): one dependent broadcast LDS read, MCF_WAVE_PROBE.  A switch of
//  its own on top of -DMCF_STAMPS, -DMCF_WAVE_STAMPS: five stamps per wave and pivot cost about 800 cycles of the loop, which
//  lane 0's phase stamps, compared between builds, must not carry)
#if defined(MCF_STAMPS) && defined(MCF_WAVE_STAMPS)
__shared__ unsigned long long mcf_wave_acc[16][6];
__shared__ unsigned long long mcf_wave_t0[16];
#define MCF_WAVE_T0() do { if ((threadIdx.x & 63) == 0) mcf_wave_t0[threadIdx.x >> 6] = __builtin_amdgcn_s_memtime(); } while (0)
#define MCF_WAVE_STAMP(slot)                                                                                                  \
    do { if ((threadIdx.x & 63) == 0) mcf_wave_acc[threadIdx.x >> 6][slot] += __builtin_amdgcn_s_memtime() - mcf_wave_t0[threadIdx.x >> 6]; } while (0)
// What one dependent broadcast read costs: three clocks, each waited for, with one LDS read of a uniform address between the
// second and the third; (c - b) - (b - a) is the read's issue, latency and wait.
#define MCF_WAVE_PROBE(word)                                                                                                  \
    do {                                                                                                                      \
        if (threadIdx.x < 64) {                                                                                               \
            const unsigned long long a_ = __builtin_amdgcn_s_memtime();                                                       \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                \
            const unsigned long long b_ = __builtin_amdgcn_s_memtime();                                                       \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                \
            const int32_t x_ = *reinterpret_cast<const volatile int32_t*>(word);                                              \
            asm volatile("s_waitcnt lgkmcnt(0)" ::"v"(x_) : "memory");                                                        \
            const unsigned long long c_ = __builtin_amdgcn_s_memtime();                                                       \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                \
            if (threadIdx.x == 0) mcf_wave_acc[0][5] += (c_ - b_) - (b_ - a_);                                                \
        }                                                                                                                     \
    } while (0)
#else
#define MCF_WAVE_T0() do {} while (0)
#define MCF_WAVE_STAMP(slot) do {} while (0)
#define MCF_WAVE_PROBE(word) do {} while (0)
#endif

// ------------------------------------------------------------------ node-parallel cycle search (LDS loop)
// A tree that fits one workgroup's lanes needs no walk at all: lane x asks whether NODE x is an ancestor of the entering arc's
// first / second end point -- pos[x] <= pos[u] < pos[x] + size[x], both from LDS -- and, if it is an ancestor of exactly one,
// files itself at path index depth[u] - depth[x] with its record and position (what the climb would have recorded) and
// takes part in that side's ratio test; the deepest common ancestor is the join.  Three dependent LDS reads and two wave
// reductions for the whole cycle, whatever its length, instead of one dependent round per tree level on one or two lanes
// (the 2-lane climb was 53 % of a pivot on netgen_8_08a).  Same path arrays, same ratio-test winners (first side: lowest
// index among equal residuals, second side: highest), hence the same pivots.  All threads call it; one barrier inside;
// every wave gets the finished McfCycle.  Lane x takes the nodes x, x + THREADS, ... (netgen_8_08a has 257 tree nodes: two
// passes at 256 lanes), so the tree need not fit the workgroup; the caller gates on kSmallCycleMaxNodes.
// After the barrier EVERY wave finishes for itself, uniformly: the per-wave counts are one LDS read per lane summed over scalar
// lane reads, each side's ratio test is one DPP min reduction per 64 path indices with the winner taken from a ballot -- two
// independent chains, which overlap only where the code makes them (small_ratio_together) -- and the join is two broadcast
// reads.  The finished cycle is then in every wave's scalar registers: no McfCycle goes through LDS, and nobody waits for wave 0
// to publish it.
// The end points' positions, depths and records come from the caller's registers (mcf_pivot_begin_t<true> read them): the
// finish pass of a faster wave may already be rewriting node[u_in] when a slower one gets here.  For the same reason the
// residuals and the by-depth table have LDS of their own (SmallLayout::scratch, 20 B per tree node) and not the segment
// table's, which the finish pass fills.
struct alignas(8) SmallCycleAcc {
    int32_t c[16][2];   // one-sided ancestors per wave, first / second side (side by side: one 8-byte read fetches a wave's pair)
};
// The join is not looked for: nothing behind the search reads it (mcf_pivot_decide: d1 / d2 / k1 / k2 / n1 / n2; mcf_pivot_swap:
// n1 / n2 and the end points' r0 / p0 / s0), so the common ancestors file nothing -- the loads of the look-up folded away on their
// own, the by-depth LDS stores could not -- and the by-depth part of the scratch goes unused.  The root, node n_nodes - 1, is a
// common ancestor at every pivot: the passes run over the real nodes only, one pass instead of two at 256 real nodes and 256
// lanes.  At 256 lanes only: at 1 024 lanes, where 257 tree nodes are one pass either way, the kernels without the join measured
// 80 - 470 cycles per pivot SLOWER than with it (profiles/small_loop_back_stamps.txt), so they keep it.
constexpr bool small_search_join(int threads) { return threads != 256; }

// Ratio test of one side over res[0 .. n), by all 64 lanes of a wave.  !LAST: strictly smaller wins, the lowest index among
// equal residuals (d = MCF_INF, k = -1 when nothing is below MCF_INF); LAST: smaller or equal wins, the highest index.
// A side whose residuals are all MCF_INF or below 2^32 - 1 (mcf_ratio_narrow_ok; one ballot over all its strides makes that a
// uniform test) is reduced on 32-bit keys: one v_min_u32 with a DPP operand per step where the 64-bit reduction takes two moves,
// a 64-bit compare and two selects.  Lanes past the end hold the key of MCF_INF and stay out of the winner's ballot.  Any other
// side takes the 64-bit reduction; d and k are the same either way (profiles/small_loop_reduce_stamps.txt).
template <bool LAST>
__device__ __forceinline__ void small_ratio_side(const int64_t* res, int32_t n, int64_t* d_out, int32_t* k_out) {
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    int64_t d = MCF_INF;
    int32_t k = -1;
    const int64_t r0 = lane < n ? res[lane] : MCF_INF;
    bool wide = !mcf_ratio_narrow_ok(r0);
    for (int32_t i = 64 + lane; i < n; i += 64) wide |= !mcf_ratio_narrow_ok(res[i]);
    if (__ballot(wide) == 0) {
        for (int32_t base = 0; base < n; base += 64) {   // (uniform, as below)
            const int32_t i = base + lane;
            const uint32_t key = mcf_ratio_key32(base == 0 ? r0 : (i < n ? res[i] : MCF_INF));
            const uint32_t mn = mcf_wave_min_u32(key);
            const uint64_t mask = __ballot(i < n && key == mn);
            mcf_ratio_take<LAST>(mcf_ratio_unkey32(mn), mask, base, d, k);
        }
        *d_out = d; *k_out = k;
        return;
    }
    for (int32_t base = 0; base < n; base += 64) {   // (uniform; one trip unless the path is longer than a wave)
        const int32_t i = base + lane;
        // lanes past the end can never hold the minimum: a residual is at most MCF_INF
        const int64_t r = i < n ? res[i] : INT64_MAX;
        const int64_t mn = -mcf_wave_max64(-r);
        const uint64_t mask = __ballot(r == mn);
        mcf_ratio_take<LAST>(mn, mask, base, d, k);
    }
    *d_out = d; *k_out = k;
}

// One branch for both sides: a one-sided ancestor picks its side's path, record, position and residual arrays and the end point's
// depth with selects on `au`, computes ONE residual -- the arc loses flow when (up arc) == (first side) -- and stores once: the same
// words with the same values as one branch per side, but a wave that holds ancestors of both end points no longer runs two
// bodies one after the other.  At 256 lanes only: the 1 024-lane front kernel measured 135 cycles per pivot SLOWER with it
// (profiles/small_loop_reduce_stamps.txt), and keeps one branch per side.
constexpr bool small_search_one_branch(int threads) { return threads == 256; }

// Both ratio tests from one round trip behind the search barrier: res1[lane] and res2[lane] are loaded beside the per-wave counts,
// and when both sides fit one stride of 64 and are narrow (mcf_ratio_narrow_ok) -- one uniform test -- the two 32-bit reductions
// run as one piece of straight-line code.  One side's load used to wait for the other side's whole reduction, behind the counts'
// round trip: three dependent trips where the data needs one.  Every other case takes small_ratio_side; winners and ties are
// mcf_ratio_take's either way.  At both widths: every wave runs the ratio tests for itself, so four waves per SIMD hide nothing of
// them either -- 1 024 lanes measured -357 / -260 / -276 cycles per pivot under rules 0 / 1 / 2 (profiles/small_loop_trips_stamps.txt).
constexpr bool small_ratio_together(int threads) { return threads == 256 || threads == 1024; }
// The search reads a node's whole record at once (see the loop).  At 256 lanes only: at 1 024 it measured nothing (-26 / +9 / +2).
constexpr bool small_record_once(int threads) { return threads == 256; }
typedef int small_i32x4 __attribute__((ext_vector_type(4)));
// The ratio tests' inputs in the one trip they need: lane w fetches wave w's pair of counts with ONE unconditional 8-byte read (the
// index clamped where an exec mask used to be: two masked reads, each with its own save and restore of exec), both residual loads
// are in flight before the wait for the counts (left alone the compiler sank them behind the branch on the counts, a second
// dependent round trip), and the 32-bit keys are made where the narrow test's compares are, so that no lane mask has to live in
// a VGPR lane across the branch into the straight-line reductions.  At 256 lanes (the 1 024-lane kernels were not measured with it).
constexpr bool small_ratio_one_trip(int threads) { return threads == 256; }
typedef int small_i32x2 __attribute__((ext_vector_type(2)));
// The slot budget, second part: the stages behind the pick counted in issue slots, in the 256-lane front
// kernels.  (Diagnostic builds switch one part off alone with -DMCF_BUDGET_OFF=<bits>: 1 pairs, 2 ballots, 4 counts, 8 the
// finish pass's loads in one trip.)
#ifndef MCF_BUDGET_OFF
#define MCF_BUDGET_OFF 0
#endif
//   side- and buffer-selected LDS addresses by arithmetic: small_plan lays the arrays of a pair a constant distance apart
//   (mcf_pair_dist4 / mcf_pair_dist16), so the second one's element is the first one's at index + bit * distance -- one 24-bit
//   multiply-add where a select between two base addresses in scalar registers is two moves and the select
constexpr bool small_pair_arith(int threads, bool front) { return threads == 256 && front && !(MCF_BUDGET_OFF & 1); }
//   ballots of the search and of the ratio tests straight from their compares, joined as lane masks in scalar registers: a
//   ballot of a bool put together with && goes through a VGPR (v_cndmask 0, 1 and a v_cmp_ne of it)
constexpr bool small_ballot_direct(int threads, bool front) { return threads == 256 && front && !(MCF_BUDGET_OFF & 2); }
//   a wave's two counts in one word (mcf_counts_pack): four lane reads, three adds and the unpacking where eight and eight stood
constexpr bool small_counts_packed(int threads, bool front) { return threads == 256 && front && !(MCF_BUDGET_OFF & 4); }
//   the pair form of the finish pass issues the first trip's loads of all four of its passes together (mcf_pivot_finish_pairs<true>)
constexpr bool small_finish_one_trip(int threads, bool front) { return small_pair_arith(threads, front) && !(MCF_BUDGET_OFF & 8); }

// `cy` as mcf_pivot_begin_t<true> left it (in registers, uniform); on return the finished cycle, uniform in every wave.
template <int THREADS, bool FRONT>
__device__ __forceinline__ void small_cycle_parallel(const McfView& v, SmallCycleAcc& A, int64_t* scratch, McfCycle& cy) {
    constexpr bool kScalar = small_scalar_control(THREADS);
    constexpr bool kSearchJoin = small_search_join(THREADS);
    constexpr bool kSearchOneBranch = small_search_one_branch(THREADS);
    constexpr bool kRatioTogether = small_ratio_together(THREADS);
    constexpr bool kRecordOnce = small_record_once(THREADS);
    constexpr bool kRatioOneTrip = kRatioTogether && small_ratio_one_trip(THREADS);
    constexpr bool kPairs = small_pair_arith(THREADS, FRONT) && kSearchOneBranch;
    constexpr bool kBallot = small_ballot_direct(THREADS, FRONT) && kSearchOneBranch && !kSearchJoin && kRatioOneTrip;
    constexpr bool kCounts = small_counts_packed(THREADS, FRONT) && kRatioOneTrip;
    const McfCtx* c = v.ctx;   // (the caller's registers)
    const int32_t d4 = mcf_pair_dist4(v.n_nodes), d16 = mcf_pair_dist16(v.n_nodes);   // (kPairs; constants of the launch)
    const int32_t* pcur = kPairs ? v.posbuf[0] + mcf_pair_index(0, c->cur, d4) : (c->cur ? v.posbuf[1] : v.posbuf[0]);
    const int32_t du0 = cy.r0u.depth, dw0 = cy.r0w.depth;
    const int32_t pu = cy.p0u, pw = cy.p0w;
    const int32_t wave = (int32_t)threadIdx.x >> 6;
    const int32_t N = v.n_nodes;
    // scratch: residual per path index and side, and the common ancestors by depth (root .. join occupy depths
    // 0 .. depth[join], one node each)
    int64_t* const res1 = scratch;
    int64_t* const res2 = res1 + N;
    int32_t* const by_depth = reinterpret_cast<int32_t*>(res2 + N);
    int32_t n1w = 0, n2w = 0;   // this wave's one-sided ancestors, over its passes
    const int32_t nx = kSearchJoin ? N : N - 1;   // (the root files nothing: see kSearchJoin)
    // (kPairs) a one-sided ancestor files itself at index depth[end point] - depth[x] of its side's arrays: with the side as a
    // number that is (du0 - depth[x]) + bit * (dw0 - du0) in the first side's terms, and the second side's arrays begin d4 / d16
    // elements behind the first's -- one multiply-add per kind of array names the element in either
    const int32_t side4 = dw0 - du0 + d4, side16 = dw0 - du0 + d16;
    auto file_pairs = [&](bool au, const McfNode& rec, int32_t px, int32_t x) {
        const McfArcW a = v.arcw[rec.pred >> 1];
        const int32_t bit = mcf_pair_bit(!au), i0 = du0 - rec.depth;
        const int32_t i4 = mcf_pair_index(i0, bit, side4), i16 = mcf_pair_index(i0, bit, side16);
        v.path1[i4] = x; v.rec1[i16] = rec; v.ppos1[i4] = px;
        const bool loses = ((rec.pred & 1) != 0) == au;
        res1[i16] = loses ? a.flow : (a.cap >= MCF_INF ? MCF_INF : a.cap - a.flow);
    };
    for (int32_t x0 = 0; x0 < nx; x0 += THREADS) {   // (uniform: every wave makes every pass)
        const int32_t x = x0 + (int32_t)threadIdx.x;
        bool h1 = false, h2 = false;
        uint64_t b1 = 0, b2 = 0;   // (kBallot) this pass's one-sided ancestors as lane masks
        if constexpr (kBallot) {
            // every lane reads -- one past the last node reads the last node's words -- so that the two ancestor tests are compares
            // of this block and the ballots take their lane masks as they stand; "inside" and "one-sided" are mask arithmetic
            const uint64_t bin = __builtin_amdgcn_ballot_w64(x < nx);
            const int32_t xi = min(x, nx - 1);
            const small_i32x4 raw = *reinterpret_cast<const small_i32x4*>(&v.node[xi]);
            McfNode rec;
            rec.parent = raw.x; rec.pred = raw.y; rec.size = raw.z; rec.depth = raw.w;
            const int32_t px = pcur[xi];
            const bool au = (uint32_t)(pu - px) < (uint32_t)rec.size, aw = (uint32_t)(pw - px) < (uint32_t)rec.size;
            const uint64_t bu = __builtin_amdgcn_ballot_w64(au) & bin, bw = __builtin_amdgcn_ballot_w64(aw) & bin;
            b1 = bu & ~bw; b2 = bw & ~bu;
            if (x < nx && au != aw) {
                if constexpr (kPairs) file_pairs(au, rec, px, x);
                else {
                    const McfArcW a = v.arcw[rec.pred >> 1];
                    const int32_t idx = (au ? du0 : dw0) - rec.depth;
                    (au ? v.path1 : v.path2)[idx] = x; (au ? v.rec1 : v.rec2)[idx] = rec; (au ? v.ppos1 : v.ppos2)[idx] = px;
                    const bool loses = ((rec.pred & 1) != 0) == au;
                    (au ? res1 : res2)[idx] = loses ? a.flow : (a.cap >= MCF_INF ? MCF_INF : a.cap - a.flow);
                }
            }
        } else if (x < nx) {
            // (kRecordOnce) the record as ONE 16-byte read beside the position: an ancestor lane then holds depth, pred and parent
            // and goes straight to its tree arc, where the fields, read one by one, came in a round trip of their own
            McfNode rec;
            if (kRecordOnce) {
                const small_i32x4 raw = *reinterpret_cast<const small_i32x4*>(&v.node[x]);
                rec.parent = raw.x; rec.pred = raw.y; rec.size = raw.z; rec.depth = raw.w;
            } else rec = v.node[x];
            const int32_t px = pcur[x];
            const bool au = (uint32_t)(pu - px) < (uint32_t)rec.size, aw = (uint32_t)(pw - px) < (uint32_t)rec.size;
            if (au && aw) { if (kSearchJoin) by_depth[rec.depth] = x; }
            else if (kSearchOneBranch) {
                if constexpr (kPairs) {
                    if (au || aw) { file_pairs(au, rec, px, x); h1 = au; h2 = aw; }
                } else if (au || aw) {
                    const McfArcW a = v.arcw[rec.pred >> 1];
                    const int32_t idx = (au ? du0 : dw0) - rec.depth;
                    (au ? v.path1 : v.path2)[idx] = x; (au ? v.rec1 : v.rec2)[idx] = rec; (au ? v.ppos1 : v.ppos2)[idx] = px;
                    // the first side is walked against the flow, the second with it: an up arc loses flow there and gains here
                    const bool loses = ((rec.pred & 1) != 0) == au;
                    (au ? res1 : res2)[idx] = loses ? a.flow : (a.cap >= MCF_INF ? MCF_INF : a.cap - a.flow);
                    h1 = au; h2 = aw;
                }
            } else if (au) {
                const McfArcW a = v.arcw[rec.pred >> 1];
                const int32_t idx = du0 - rec.depth;
                v.path1[idx] = x; v.rec1[idx] = rec; v.ppos1[idx] = px;
                // first side is walked against the flow: an up arc loses flow, a down arc gains
                res1[idx] = (rec.pred & 1) ? a.flow : (a.cap >= MCF_INF ? MCF_INF : a.cap - a.flow);
                h1 = true;
            } else if (aw) {
                const McfArcW a = v.arcw[rec.pred >> 1];
                const int32_t idx = dw0 - rec.depth;
                v.path2[idx] = x; v.rec2[idx] = rec; v.ppos2[idx] = px;
                res2[idx] = (rec.pred & 1) ? (a.cap >= MCF_INF ? MCF_INF : a.cap - a.flow) : a.flow;
                h2 = true;
            }
        }
        n1w += (int32_t)__popcll(kBallot ? b1 : (uint64_t)__ballot(h1));
        n2w += (int32_t)__popcll(kBallot ? b2 : (uint64_t)__ballot(h2));
    }
    if ((threadIdx.x & 63) == 0) {
        if (kCounts) A.c[wave][0] = (int32_t)mcf_counts_pack(n1w, n2w);   // (one word: the second of the wave's pair goes unused)
        else { A.c[wave][0] = n1w; A.c[wave][1] = n2w; }
    }
    MCF_WAVE_STAMP(0);
    __syncthreads();   // path / record / residual / by_depth entries and the per-wave counts -> every wave's ratio tests, its
                       // decision and the finish pass
    int32_t n1 = 0, n2 = 0;
    int64_t d1, d2;
    int32_t k1, k2;
    {
        constexpr int kWaves = THREADS / 64;
        const int32_t lane = (int32_t)(threadIdx.x & 63);
        // one read, then scalar lane reads (of the lanes below kWaves only: the others may hold anything)
        int32_t c1, c2;
        if (kCounts) {
            c1 = A.c[lane < kWaves ? lane : kWaves - 1][0]; c2 = 0;
        } else if (kRatioOneTrip) {
            const small_i32x2 cc = *reinterpret_cast<const small_i32x2*>(&A.c[lane < kWaves ? lane : kWaves - 1][0]);
            c1 = cc.x; c2 = cc.y;
        } else {
            c1 = lane < kWaves ? A.c[lane][0] : 0; c2 = lane < kWaves ? A.c[lane][1] : 0;
        }
        // (kRatioTogether) both sides' first residuals ride in the same round trip as the counts: their addresses do not hang on
        // the counts, only their masking does.  A lane past the scratch's end reads its last word; past a side's end, a word
        // the search of an earlier pivot left there, or nothing anybody wrote: either is masked below.
        const int32_t li = lane < N ? lane : N - 1;
        int64_t q1 = 0, q2 = 0;
        if (kRatioTogether) { q1 = res1[li]; q2 = res2[li]; }
        // (the counts and both residuals wanted here: all three reads are issued before the one wait)
        if (kRatioOneTrip) asm volatile("" ::"v"(c1), "v"(c2), "v"(q1), "v"(q2));
        if (kCounts) {
            uint32_t sum = 0;   // (no carry from the first side's half into the second's: mcf_counts_pack)
#pragma unroll
            for (int q = 0; q < kWaves; ++q) sum += (uint32_t)__builtin_amdgcn_readlane(c1, q);
            n1 = mcf_counts_first(sum); n2 = mcf_counts_second(sum);
        } else {
#pragma unroll
            for (int q = 0; q < kWaves; ++q) { n1 += __builtin_amdgcn_readlane(c1, q); n2 += __builtin_amdgcn_readlane(c2, q); }
        }
        // the ratio tests, exactly the climb's: first side -- strictly smaller wins (lowest index among equals), second side --
        // smaller or equal wins (highest index among equals)
        bool both = false;
        if constexpr (kBallot) {
            // the same tests on the loaded words: a lane is IN its side, its residual FINITE, or WIDE -- r = in ? q : MCF_INF is never
            // formed; each ballot is of one compare, and the lane masks are joined in scalar registers
            const bool in1 = lane < n1, in2 = lane < n2, f1 = q1 != MCF_INF, f2 = q2 != MCF_INF;
            uint32_t key1 = (in1 && f1) ? (uint32_t)q1 : 0xffffffffu, key2 = (in2 && f2) ? (uint32_t)q2 : 0xffffffffu;   // (mcf_ratio_key32)
            asm volatile("" : "+v"(key1), "+v"(key2));
            const uint64_t m1 = __builtin_amdgcn_ballot_w64(in1), m2 = __builtin_amdgcn_ballot_w64(in2);
            const uint64_t odd = (m1 & __builtin_amdgcn_ballot_w64(f1) & __builtin_amdgcn_ballot_w64((uint64_t)q1 > 0xfffffffeull)) |
                                 (m2 & __builtin_amdgcn_ballot_w64(f2) & __builtin_amdgcn_ballot_w64((uint64_t)q2 > 0xfffffffeull));
            both = n1 <= 64 && n2 <= 64 && odd == 0;
            if (both) {
                uint32_t mn1, mn2;
                mcf_wave_min_u32_pair(key1, key2, mn1, mn2);
                const uint64_t mask1 = m1 & __builtin_amdgcn_ballot_w64(key1 == mn1), mask2 = m2 & __builtin_amdgcn_ballot_w64(key2 == mn2);
                d1 = MCF_INF; k1 = -1; d2 = MCF_INF; k2 = -1;
                if (n1 > 0) mcf_ratio_take<false>(mcf_ratio_unkey32(mn1), mask1, 0, d1, k1);
                if (n2 > 0) mcf_ratio_take<true>(mcf_ratio_unkey32(mn2), mask2, 0, d2, k2);
            }
        } else if (kRatioTogether) {
            const int64_t r1 = lane < n1 ? q1 : MCF_INF, r2 = lane < n2 ? q2 : MCF_INF;
            // ONE uniform test: both sides fit one stride and are narrow.  Then the two 32-bit reductions are straight-line code
            // with nothing between them, and their DPP steps interleave.
            const bool odd = !mcf_ratio_narrow_ok(r1) || !mcf_ratio_narrow_ok(r2);
            uint32_t key1 = mcf_ratio_key32(r1), key2 = mcf_ratio_key32(r2);
            if (kRatioOneTrip) asm volatile("" : "+v"(key1), "+v"(key2));   // (made here, beside the narrow test's compares)
            both = n1 <= 64 && n2 <= 64 && __ballot(odd) == 0;
            if (both) {
                uint32_t mn1, mn2;
                mcf_wave_min_u32_pair(key1, key2, mn1, mn2);
                const uint64_t mask1 = __ballot(lane < n1 && key1 == mn1), mask2 = __ballot(lane < n2 && key2 == mn2);
                d1 = MCF_INF; k1 = -1; d2 = MCF_INF; k2 = -1;
                // (an empty side takes nothing, as the loop over its strides: its mask is empty)
                if (n1 > 0) mcf_ratio_take<false>(mcf_ratio_unkey32(mn1), mask1, 0, d1, k1);
                if (n2 > 0) mcf_ratio_take<true>(mcf_ratio_unkey32(mn2), mask2, 0, d2, k2);
            }
        }
        if (!both) {   // a side longer than a stride, a wide residual or a negative one
            small_ratio_side<false>(res1, n1, &d1, &k1);
            small_ratio_side<true>(res2, n2, &d2, &k2);
        }
    }
    cy.d1 = uni64<kScalar>(d1); cy.k1 = uni32<kScalar>(k1); cy.d2 = uni64<kScalar>(d2); cy.k2 = uni32<kScalar>(k2);
    cy.n1 = n1; cy.n2 = n2;
    MCF_WAVE_STAMP(1);
    if (kSearchJoin) {
        const int32_t jn = uni32<kScalar>(by_depth[du0 - n1]);   // the join: the common ancestor right above the first side's path
        const McfNode rj = uni_node<kScalar>(v.node[jn]);        // (the finish pass leaves the join's record alone)
        const int32_t pj = uni32<kScalar>(pcur[jn]);
        cy.u = jn; cy.w = jn; cy.ru = rj; cy.rw = rj;
        cy.pu = pj; cy.pw = pj; cy.su = pj; cy.sw = pj;
    }
    // (p0u / p0w / s0u / s0w / r0u / r0w stay what mcf_pivot_begin_t<true> read)
}

// ------------------------------------------------------------------ pricing sweep of the LDS loop
// The sweep is specialised at compile time and chosen once per launch, so that its inner loop tests neither the rule nor
// the key mode: kSweepPlain -- Dantzig / candidate list with the plain key (the violation), kSweepDevex -- the Devex merit
// with the direction-carrying id, kSweepGeneric -- everything else (the specialised key modes of mcf_dantzig_key).
enum { kSweepGeneric = 0, kSweepPlain = 1, kSweepDevex = 2 };

// One arc priced from the LDS arrays: state, end points, cost and id in one round trip, the two potentials in a second.
template <int MODE>
__device__ __forceinline__ void small_price_lds(const McfView& v, int32_t rule, bool devex, int32_t i, int64_t& key, int64_t& arc) {
    const int32_t st = v.state[i];
    const int32_t t = v.tail[i], h = v.head[i], o = v.orig[i];
    const int64_t cst = v.cost[i];
    float w = 1.0f;
    if (MODE == kSweepDevex || (MODE == kSweepGeneric && rule == MCF_RULE_DEVEX_BLOCK)) w = v.weight[i];
    const int64_t rc = cst + v.pi[t] - v.pi[h];
    const int64_t viol = st > 0 ? -rc : rc;
    if (st == 0 || viol <= 0) return;
    int64_t kk;
    int32_t id = o;
    if (MODE == kSweepPlain) kk = viol;
    else if (MODE == kSweepDevex) {
        kk = __double_as_longlong(((double)viol * (double)viol) / (double)w);
        id = mcf_devex_tie_id(o, st);
    } else {
        kk = mcf_dantzig_key(v, i, viol, st);
        if (rule == MCF_RULE_DEVEX_BLOCK) kk = __double_as_longlong(((double)viol * (double)viol) / (double)w);
        if (devex) id = mcf_devex_tie_id(o, st);
    }
    const int64_t pid = mcf_pack_arc(id, i);
    if (mcf_cand_better(kk, pid, key, arc)) { key = kk; arc = pid; }
}

// Arg-max inside each half of a wave (32 lanes = one head bucket at 256 lanes): the first five DPP steps of
// mcf_wave_max64 leave the max of rows 0-1 in lane 31 and of rows 2-3 in lane 63; ids as in wave_argmax.  The result is
// uniform per half.  All 64 lanes must be active.
__device__ __forceinline__ void half_wave_argmax(int64_t& key, int64_t& arc) {
    int64_t x = key;
    x = mcf_dpp_max_step<0xB1, 0xf>(x);
    x = mcf_dpp_max_step<0x4E, 0xf>(x);
    x = mcf_dpp_max_step<0x141, 0xf>(x);
    x = mcf_dpp_max_step<0x140, 0xf>(x);
    x = mcf_dpp_max_step<0x142, 0xa>(x);
    const int64_t m0 = readlane64(x, 31), m1 = readlane64(x, 63);
    const bool upper = (threadIdx.x & 32) != 0;
    const int64_t mx = upper ? m1 : m0;
    const uint64_t mask = __ballot(key == mx && key > 0);
    int64_t best[2] = {-1, -1};
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        uint64_t mk = hf ? (mask >> 32) << 32 : mask & 0xffffffffull;
        while (mk) {  // uniform loop: one iteration unless several lanes tie on the key
            const int lane = __ffsll((unsigned long long)mk) - 1;
            const int64_t a = readlane64(arc, lane);
            if (best[hf] < 0 || a < best[hf]) best[hf] = a;
            mk &= mk - 1;
        }
    }
    const int64_t b = upper ? best[1] : best[0];
    key = b < 0 ? 0 : mx;
    arc = b;
}

// ---- the front of a pivot on the plain register sweep: 32-bit keys, and an arg-max that hands the candidate over.
// The pivot descriptor in the LDS image: at 256 lanes the kernels carry it in registers across the loop and lane 0 stores it once
// behind the loop (small_desc_store_all: -280 to -340 cycles per pivot under Devex and the candidate list, 0 B scratch; the front
// kernel 2.90 -> 2.81 us per pivot against the same fourteen stores moved to wave 1, which neither holds the apply positions
// lo .. lo + 63 nor finishes, and 3.00 with them in wave 0: profiles/small_loop_decide_parts.txt).  The 1 024-lane kernels keep
// lane 0's per-pivot stores (small_desc_store): carrying the descriptor spilled there (profiles/small_loop_back_stamps.txt).
constexpr bool small_desc_once(int threads, bool front) { return threads == 256; }
// The straight-line decide (mcf_pivot_decide_flat: selects where mcf_pivot_decide returns early) where the control block lives in
// vector registers and the kernel never carries Devex weights: the 256-lane front kernel.
constexpr bool small_decide_flat(int threads, bool front) { return threads == 256 && front; }
// The loop budgeted in issue slots ("The slot budget"): at 256 lanes a wave is alone on its SIMD and pays for
// every instruction it issues, waits for VCC included.  Each part has a switch of its own; the 1 024-lane kernels keep the forms
// they were measured with.
//   the narrow register sweep without compares for the violation, on kPriceChains accumulators (front kernels price narrow)
constexpr bool small_price_flat(int threads, bool front) { return threads == 256 && front; }
constexpr int small_price_chains(int threads, bool front) { return small_price_flat(threads, front) ? 2 : 1; }
//   the arg-max's pick reads the waves' 16-byte slots whole, in one round trip, and unpacks with selects
constexpr bool small_pick_one_trip(int threads) { return threads == 256; }
// What a lane remembers of its best arc besides the key: end points and slot in one word -- tail | head << 11 | slot << 22,
// slot q = the lane's q-th arc, engine index r_lo + q * r_step (the lanes' stride: THREADS under the even deal) -- the invariant
// part precomputed per register arc; bit 31 is the state's sign (set: -1, the arc sits at capacity).  11 bits per node and 9 per slot cover every instance of the LDS plan
// (small_plan: fewer than 1 371 tree nodes and 7 314 padded arcs, so at most 229 arcs per lane); small_info_fits is the
// host's check of exactly that.
__device__ __forceinline__ uint32_t small_info(int32_t tail, int32_t head, int32_t q) { return (uint32_t)tail | ((uint32_t)head << 11) | ((uint32_t)q << 22); }
// the candidate record of the winner: its key is the violation (plain sweep), so rc = -state * violation, exactly
__device__ __forceinline__ McfCandX small_record(uint32_t info, int64_t viol, int32_t orig, int32_t e) {
    McfCandX x;
    x.state = (info >> 31) ? -1 : 1;
    x.rc = x.state > 0 ? -viol : viol;
    x.arc = mcf_pack_arc(orig, e);
    x.tail = (int32_t)(info & 0x7ff); x.head = (int32_t)((info >> 11) & 0x7ff); x.pad = 0;
    return x;
}
// One arc beyond the register slots priced from LDS with the packed 32-bit key; q as in small_info
__device__ __forceinline__ void small_price_lds_narrow(const McfView& v, int32_t i, int32_t q, uint64_t& best, uint32_t& info) {
    const int32_t st = v.state[i];
    const int32_t t = v.tail[i], h = v.head[i], o = v.orig[i];
    const int32_t* pi32 = reinterpret_cast<const int32_t*>(v.pi);   // low words: exact in 32 bits under mcf_small_narrow_fits
    const int32_t rc = (int32_t)((uint32_t)v.cost[i] + (uint32_t)pi32[2 * t] - (uint32_t)pi32[2 * h]);
    const int32_t viol = st > 0 ? -rc : rc;
    const uint64_t p = ((uint64_t)(uint32_t)((st != 0 && viol > 0) ? viol : 0) << 32) | (uint32_t)~o;
    if (p > best) { best = p; info = small_info(t, h, q) | ((uint32_t)st & 0x80000000u); }
}
// Per-wave slot of the handing-over arg-max, one 16-byte read: the wave's best packed key (high word 0: none), the winner's
// engine index and its info word.  Violation, id, end points, state and the exact reduced cost all unpack from these.
struct alignas(16) SmallWaveSlot {
    uint64_t key;
    int32_t e;
    uint32_t info;
};

// ---- the control block in registers (LDS loop), on a dense view without resident reduced costs.
// Control state: every McfCtx field that mcf_pivot_begin_t, mcf_pivot_decide or the loop itself changes AND a later pivot
// reads -- carried in scalar registers across the loop, written back once after it (small_ctx_store).
#define MCF_SMALL_CTL_32(F)                                                                                                   \
    F(status) F(unbounded_arc) F(empty_blocks) F(num_blocks) F(block_granules) F(tn_total) F(tn_degenerate)                   \
    F(swaps_since_reset) F(wlist_n) F(wreset) F(minor_left) F(cur) F(pending_flip) F(prev_lo) F(prev_hi) F(apply) F(lo) F(hi) \
    F(nchg) F(stage) F(arena) F(rebuild)
#define MCF_SMALL_CTL_64(F)                                                                                                   \
    F(pivots) F(degenerate) F(bound_flips) F(arcs_priced) F(nodes_moved) F(subtree_nodes) F(cycle_arcs) F(block_size)         \
    F(block_index) F(tn_last_adapt) F(minor_pivots) F(major_sweeps)
// The descriptor of ONE pivot: written by begin / decide, read by that pivot's finish and apply passes, dead afterwards.  In
// registers only while the pivot lasts; lane 0 copies it into the LDS image as the pivot is decided (small_desc_store: stores
// nobody waits for), so that the control block a launch leaves behind is the one the other paths leave.
#define MCF_SMALL_DESC_BEGIN_32(F) F(pv_e) F(pv_s) F(pv_first) F(pv_second) F(pv_t2n)
#define MCF_SMALL_DESC_BEGIN_64(F) F(pv_rc) F(pv_cap) F(pv_flow)
#define MCF_SMALL_DESC_DECIDE_32(F) F(pv_n1) F(pv_n2) F(pv_result)
#define MCF_SMALL_DESC_DECIDE_64(F) F(pv_delta)
#define MCF_SMALL_DESC_SWAP_32(F)                                                                                             \
    F(pv_k) F(pv_vin) F(pv_leave) F(pv_leave_state) F(pv_tail_in_t2) F(pv_vin_depth) F(pv_dd0) F(t2_old) F(t2_new) F(t2_size)  \
    F(nseg)
#define MCF_SMALL_DESC_SWAP_64(F) F(sigma)
template <bool SCALAR> __device__ __forceinline__ void small_ctx_uniform(McfCtx& x) {
#define MCF_F32(f) x.f = uni32<SCALAR>(x.f);
#define MCF_F64(f) x.f = uni64<SCALAR>(x.f);
    MCF_SMALL_CTL_32(MCF_F32) MCF_SMALL_CTL_64(MCF_F64)
    MCF_SMALL_DESC_BEGIN_32(MCF_F32) MCF_SMALL_DESC_BEGIN_64(MCF_F64)
    MCF_SMALL_DESC_DECIDE_32(MCF_F32) MCF_SMALL_DESC_DECIDE_64(MCF_F64)
    MCF_SMALL_DESC_SWAP_32(MCF_F32) MCF_SMALL_DESC_SWAP_64(MCF_F64)
    x.pv_t2node = uni32<SCALAR>(x.pv_t2node);
#undef MCF_F32
#undef MCF_F64
}
#define MCF_FST(f) c->f = x.f;
__device__ __forceinline__ void small_ctx_store(McfCtx* c, const McfCtx& x) {
    MCF_SMALL_CTL_32(MCF_FST) MCF_SMALL_CTL_64(MCF_FST)
}
// What mcf_pivot_begin_t (on a candidate) and mcf_pivot_decide store, under the conditions they store it: decide leaves at
// once on an unbounded cycle (the status then says so), writes the swap's fields for a basis swap only, and the preview of a
// one-node T2 (with the first end point's adjacency range -- here never fetched: the launch's constant) only for such a T2.
__device__ __forceinline__ void small_desc_store(McfCtx* c, const McfCtx& x, int64_t adj2, int64_t adj3) {
    MCF_SMALL_DESC_BEGIN_32(MCF_FST) MCF_SMALL_DESC_BEGIN_64(MCF_FST)
    if (x.status != MCF_RUNNING) return;
    MCF_SMALL_DESC_DECIDE_32(MCF_FST) MCF_SMALL_DESC_DECIDE_64(MCF_FST)
    if (x.stage != 2) return;
    MCF_SMALL_DESC_SWAP_32(MCF_FST) MCF_SMALL_DESC_SWAP_64(MCF_FST)
    if (x.pv_t2n) {
        c->pv_t2node = x.pv_t2node;
        if (x.pv_result != 1) { c->pv_adj[0] = adj2; c->pv_adj[1] = adj3; }
    }
}
// The whole descriptor at once, after the loop (kDescOnce): cx starts as a copy of the image, and begin / decide / swap change
// exactly the fields small_desc_store copies under exactly its conditions, so the image ends up the same.
__device__ __forceinline__ void small_desc_store_all(McfCtx* c, const McfCtx& x) {
    MCF_SMALL_DESC_BEGIN_32(MCF_FST) MCF_SMALL_DESC_BEGIN_64(MCF_FST)
    MCF_SMALL_DESC_DECIDE_32(MCF_FST) MCF_SMALL_DESC_DECIDE_64(MCF_FST)
    MCF_SMALL_DESC_SWAP_32(MCF_FST) MCF_SMALL_DESC_SWAP_64(MCF_FST)
    c->pv_t2node = x.pv_t2node; c->pv_adj[0] = x.pv_adj[0]; c->pv_adj[1] = x.pv_adj[1];
}
#undef MCF_FST
template <bool SCALAR> __device__ __forceinline__ void uni_cycle(McfCycle& y) {
    y.d1 = uni64<SCALAR>(y.d1); y.d2 = uni64<SCALAR>(y.d2); y.k1 = uni32<SCALAR>(y.k1); y.k2 = uni32<SCALAR>(y.k2); y.n1 = uni32<SCALAR>(y.n1); y.n2 = uni32<SCALAR>(y.n2);
    y.u = uni32<SCALAR>(y.u); y.w = uni32<SCALAR>(y.w); y.pu = uni32<SCALAR>(y.pu); y.pw = uni32<SCALAR>(y.pw); y.su = uni32<SCALAR>(y.su); y.sw = uni32<SCALAR>(y.sw);
    y.ru = uni_node<SCALAR>(y.ru); y.rw = uni_node<SCALAR>(y.rw); y.p0u = uni32<SCALAR>(y.p0u); y.p0w = uni32<SCALAR>(y.p0w); y.s0u = uni32<SCALAR>(y.s0u); y.s0w = uni32<SCALAR>(y.s0w);
    y.r0u = uni_node<SCALAR>(y.r0u); y.r0w = uni_node<SCALAR>(y.r0w); y.small = uni32<SCALAR>(y.small);
}

// ------------------------------------------------------------------ the stages of solve_small_body, in the order it runs them
// The view of the LDS image: every array the loop follows points into `smem`; what it never follows is nulled, which folds
// the branches on it away.
template <bool FRONT>
__device__ __forceinline__ McfView small_map_view(const McfView& g, const SmallLayout& L, char* smem) {
    McfView v = g;
    v.tail = reinterpret_cast<const int32_t*>(smem + L.tail);
    v.head = reinterpret_cast<const int32_t*>(smem + L.head);
    v.cost = reinterpret_cast<const int32_t*>(smem + L.cost);
    v.orig = reinterpret_cast<const int32_t*>(smem + L.orig);
    v.state = reinterpret_cast<int8_t*>(smem + L.state);
    v.weight = g.weight ? reinterpret_cast<float*>(smem + L.weight) : nullptr;
    v.arcw = reinterpret_cast<McfArcW*>(smem + L.arcw);
    v.pi = reinterpret_cast<int64_t*>(smem + L.pi);
    v.node = reinterpret_cast<McfNode*>(smem + L.node);
    v.order[0] = reinterpret_cast<int32_t*>(smem + L.order0);
    v.order[1] = reinterpret_cast<int32_t*>(smem + L.order1);
    v.path1 = reinterpret_cast<int32_t*>(smem + L.path1);
    v.path2 = reinterpret_cast<int32_t*>(smem + L.path2);
    v.ppos1 = reinterpret_cast<int32_t*>(smem + L.ppos1);
    v.ppos2 = reinterpret_cast<int32_t*>(smem + L.ppos2);
    v.rec1 = reinterpret_cast<McfNode*>(smem + L.rec1);
    v.rec2 = reinterpret_cast<McfNode*>(smem + L.rec2);
    v.seg = reinterpret_cast<McfSeg*>(smem + L.seg);
    v.ctx = reinterpret_cast<McfCtx*>(smem + L.ctx);
    v.posbuf[0] = reinterpret_cast<int32_t*>(smem + L.pos0);
    v.posbuf[1] = reinterpret_cast<int32_t*>(smem + L.pos1);
    v.psz[0] = nullptr;  // always the climb here (see the pivot step); mcf_create keeps no sizes for such a handle
    v.psz[1] = nullptr;
    v.reach = nullptr;
    v.bmeta[0] = nullptr; v.bmeta[1] = nullptr; v.candx = nullptr; v.dirty = nullptr; v.dirty_hdr = nullptr;   // (folds the blocked list etc. away)
    v.rcache = nullptr; v.adj_off = nullptr;   // (a handle on this path keeps no resident reduced costs, mcf_create: folds their branches away)
    // the front kernel is Dantzig's: no weights, no Devex state (small_front_for refuses a view that carries weights) -- the
    // Devex branches of mcf_pivot_decide and of the finish pass fold away
    if constexpr (FRONT) { v.weight = nullptr; v.dx = nullptr; }
    return v;
}

// The image's arrays, one list for both ways: IN copies all of them into LDS, !IN copies back those a launch can change (the
// arcs' end points, costs and ids never do).
// (All fourteen arrays' loads in flight together -- one fused loop, 4- or 16-byte loads -- was measured SLOWER than these
//  plain loops: 131 / 125 us against 117 us per 20-pivot launch.)
struct SmallSizes { uint32_t m_pad4, m_padb, N, arcw_b; };   // bytes of a 4-byte and a 1-byte arc array, tree nodes, bytes of arcw
__device__ __forceinline__ SmallSizes small_sizes(const McfView& g) {
    SmallSizes z;
    z.m_pad4 = (uint32_t)((g.m + 1023) / 1024 * 1024) * 4u;
    z.m_padb = z.m_pad4 >> 2;
    z.N = (uint32_t)g.n_nodes;
    z.arcw_b = (uint32_t)(g.m + z.N - 1) * 16u;
    return z;
}
template <int THREADS, bool IN>
__device__ __forceinline__ void small_copy_image(const McfView& g, const SmallLayout& L, char* smem, bool weights, const SmallSizes& z) {
    const uint32_t m_pad4 = z.m_pad4, m_padb = z.m_padb, N = z.N, arcw_b = z.arcw_b;
    auto both = [&](void* glob, uint32_t off, uint32_t bytes) {
        if (IN) copy_words<THREADS>(smem + off, glob, bytes);
        else copy_words<THREADS>(glob, smem + off, bytes);
    };
    if (IN) {
        copy_words<THREADS>(smem + L.tail, g.tail, m_pad4);
        copy_words<THREADS>(smem + L.head, g.head, m_pad4);
        copy_words<THREADS>(smem + L.cost, g.cost, m_pad4);
        copy_words<THREADS>(smem + L.orig, g.orig, m_pad4);
    }
    both(g.state, L.state, m_padb);
    if (weights) both(g.weight, L.weight, m_pad4);
    both(g.arcw, L.arcw, arcw_b);
    both(g.pi, L.pi, N * 8u);
    both(g.node, L.node, N * 16u);
    both(g.order[0], L.order0, N * 4u);
    both(g.order[1], L.order1, N * 4u);
    both(g.posbuf[0], L.pos0, N * 4u);
    both(g.posbuf[1], L.pos1, N * 4u);
    both(g.ctx, L.ctx, (uint32_t)sizeof(McfCtx));
}

// Devex: the host-made granule table in LDS (blocks move and resize under the tuner); other rules: whole buckets
template <int THREADS>
__device__ __forceinline__ void small_load_granules(const McfView& g, bool devex, int32_t (&gran)[MCF_NUM_BUCKETS][MCF_GRANULES + 1]) {
    if (devex) {
        for (int q = threadIdx.x; q < MCF_NUM_BUCKETS * (MCF_GRANULES + 1); q += THREADS)
            (&gran[0][0])[q] = (&g.dx->gran[0][0])[q];
    } else if (threadIdx.x < MCF_NUM_BUCKETS) {
        gran[threadIdx.x][0] = (int32_t)g.bucket_off[threadIdx.x];
        gran[threadIdx.x][MCF_GRANULES] = (int32_t)g.bucket_off[threadIdx.x + 1];
    }
}
// arcs one sweep prices: over the eight buckets, the arcs below each granule boundary (Devex: the block's share follows from
// two entries; other rules sweep whole buckets: a constant of the launch)
__device__ __forceinline__ void small_sum_granules(bool devex, const int32_t (&gran)[MCF_NUM_BUCKETS][MCF_GRANULES + 1],
                                                   int32_t (&gsum)[MCF_GRANULES + 1]) {
    if (threadIdx.x <= MCF_GRANULES && (devex || threadIdx.x == 0 || threadIdx.x == MCF_GRANULES)) {
        int32_t sum = 0;
        for (int x = 0; x < MCF_NUM_BUCKETS; ++x) sum += gran[x][threadIdx.x];
        gsum[threadIdx.x] = sum;
    }
}

// ---- arg-max (the front kernels), handing the winner over.  32-bit keys: no tie loop; the winning lane writes the wave's
// slot -- packed key, engine index, info word: 16 bytes.  After the caller's one barrier every wave reads the slots by broadcast
// and picks the winner itself with plain compares -- no second reduction -- and unpacks the candidate record (wx) begin would
// otherwise look up.  The slots are rewritten by the next iteration's arg-max, which the apply barrier (or the barrier of an
// iteration that pivots on nothing) orders behind these reads.
__device__ __forceinline__ void small_handover_publish(uint64_t nbest, int64_t arc, uint32_t info, SmallWaveSlot* slot) {
    const int32_t lane = (int32_t)(threadIdx.x & 63), wave = (int32_t)(threadIdx.x >> 6);
    // in 32-bit stages: the largest violation; if one lane holds it, that lane wins, else the largest ~id among the
    // lanes that do.  The winner's own packed key IS the 64-bit maximum.
    const uint32_t vmx = mcf_wave_max_u32(mcf_argmax_viol(nbest));
    const bool any = vmx != 0;
    bool win = mcf_argmax_viol(nbest) == vmx;
    const uint64_t tied = __ballot(win);
    if (any && (tied & (tied - 1))) {   // (uniform: several lanes share the violation)
        const uint32_t imx = mcf_wave_max_u32(mcf_argmax_second(nbest, vmx));
        win = win && (uint32_t)nbest == imx;
    }
    if (any ? win : lane == 0) slot[wave] = SmallWaveSlot{any ? nbest : 0, (int32_t)(arc & 0xffffffff), info};
}
template <int THREADS>
__device__ __forceinline__ void small_handover_pick(const SmallWaveSlot* slot, int64_t& key, int64_t& arc, McfCandX& wx) {
    constexpr int kWaves = THREADS / 64;
    constexpr bool kScalar = small_scalar_control(THREADS);
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    SmallWaveSlot b;
    if constexpr (kWaves <= 4 && small_pick_one_trip(THREADS)) {
        // every slot whole, 16 bytes a read, and every word wanted here: left alone, the compiler reads the keys, branches on
        // "any" and only then reads the winner's other half -- a second dependent round trip behind the barrier
        // The words as mcf_narrow_pick wants them are the slot's own layout; the reads are of another type than the publish
        // store's, and it is the caller's barrier between the two, not the types, that orders them behind it.
        static_assert(sizeof(SmallWaveSlot) == 16 && offsetof(SmallWaveSlot, key) == 0 && offsetof(SmallWaveSlot, e) == 8 &&
                      offsetof(SmallWaveSlot, info) == 12, "key low, key high, engine index, info word: four words of a 16-byte read");
        typedef uint32_t pick_u32x4 __attribute__((ext_vector_type(4)));
        pick_u32x4 raw[kWaves];
#pragma unroll
        for (int q = 0; q < kWaves; ++q) raw[q] = reinterpret_cast<const pick_u32x4*>(slot)[q];
        static_assert(kWaves == 4, "the one statement below names every slot: one wait for all four reads");
        asm volatile("" : "+v"(raw[0]), "+v"(raw[1]), "+v"(raw[2]), "+v"(raw[3]));
        uint32_t w[kWaves][4];
#pragma unroll
        for (int q = 0; q < kWaves; ++q) { w[q][0] = raw[q].x; w[q][1] = raw[q].y; w[q][2] = raw[q].z; w[q][3] = raw[q].w; }
        mcf_narrow_pick<kWaves>(w, key, arc, wx);
        key = uni64<kScalar>(key); arc = uni64<kScalar>(arc);
        wx.rc = uni64<kScalar>(wx.rc); wx.tail = uni32<kScalar>(wx.tail); wx.head = uni32<kScalar>(wx.head); wx.state = uni32<kScalar>(wx.state);
        return;
    } else if constexpr (kWaves <= 4) {   // one round trip, kWaves reads
        SmallWaveSlot sl[kWaves];
#pragma unroll
        for (int q = 0; q < kWaves; ++q) sl[q] = slot[q];
        b = sl[0];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) if (sl[q].key > b.key) b = sl[q];
    } else {   // sixteen waves: lane q takes slot q, one more max names the winning lane, scalar lane reads fetch the rest
        const SmallWaveSlot mine = slot[lane < kWaves ? lane : 0];
        const uint64_t k = lane < kWaves ? mine.key : 0;
        b.key = (uint64_t)mcf_wave_max64((int64_t)k);
        const int32_t w = (int32_t)__builtin_ctzll((unsigned long long)__ballot(k == b.key));
        b.e = __builtin_amdgcn_readlane(mine.e, w);
        b.info = (uint32_t)__builtin_amdgcn_readlane((int32_t)mine.info, w);
    }
    key = (int64_t)(b.key >> 32);
    if (key > 0) {
        wx = small_record(b.info, key, (int32_t)~(uint32_t)b.key, b.e);
        arc = wx.arc;
    } else { key = 0; arc = -1; }
    key = uni64<kScalar>(key); arc = uni64<kScalar>(arc);
    wx.rc = uni64<kScalar>(wx.rc); wx.tail = uni32<kScalar>(wx.tail); wx.head = uni32<kScalar>(wx.head); wx.state = uni32<kScalar>(wx.state);
}

// ---- cycle search: the end points as begin read them, uniform, and every running field of the cycle started at them
template <bool SCALAR> __device__ __forceinline__ void small_cycle_ends(McfCycle& cy) {
    cy.r0u = uni_node<SCALAR>(cy.r0u); cy.r0w = uni_node<SCALAR>(cy.r0w);
    cy.ru = cy.r0u; cy.rw = cy.r0w;
    cy.p0u = uni32<SCALAR>(cy.p0u); cy.p0w = uni32<SCALAR>(cy.p0w);
    cy.s0u = cy.p0u; cy.s0w = cy.p0w; cy.pu = cy.p0u; cy.pw = cy.p0w; cy.su = cy.p0u; cy.sw = cy.p0w;
}
// ---- apply: block permutation of the preorder array + potential shift, the descriptor straight from registers, the
// sources from the recorded stem (mcf_apply_source_paths)
// The catch-up over [prev_lo, prev_hi) outside [lo, hi) copies order[cur][j] into order[cur ^ 1][j] and pos[cur ^ 1]: other j and
// other nodes than the first loop's, and order[cur] is written by nobody between these two barriers.  So its first trip's read
// is issued in front of the first loop (kCatchUpBeside) and only its stores follow it, where the whole loop used to start --
// with a round trip of its own -- when the first one had ended.  In the 256-lane front kernel only: the general kernel measured
// some 200 cycles per pivot SLOWER with it under Devex, and 1 024 lanes measured 0 (profiles/small_loop_trips_stamps.txt).
constexpr bool small_catch_up_beside(int threads, bool front) { return threads == 256 && front; }
template <int THREADS, bool FRONT> __device__ __forceinline__ void small_apply(const McfView& v, const McfCtx& cx) {
    if (!cx.apply) return;
    constexpr bool kCatchUpBeside = small_catch_up_beside(THREADS, FRONT);
    const int32_t lo = cx.lo, hi = cx.hi, plo = cx.prev_lo, phi = cx.prev_hi;
    const int32_t jc = plo + (int32_t)threadIdx.x;   // the catch-up's first trip
    const bool catch0 = kCatchUpBeside && jc < phi && (jc < lo || jc >= hi);
    int32_t ndc = 0;
    if constexpr (small_pair_arith(THREADS, FRONT)) {
        // the leaving side and the two buffers as numbers -- a swap's pv_result is 1 or 2, cur is 0 or 1 -- times the pairs'
        // distances, where five base addresses were selected (mcf_apply_one_paths_at: the same pass on addresses named here)
        const int32_t d4 = mcf_pair_dist4(v.n_nodes), d16 = mcf_pair_dist16(v.n_nodes);
        const int32_t sbit = cx.pv_result - 1, nbit = cx.cur ^ 1;
        const McfNode* const srec = v.rec1 + mcf_pair_index(0, sbit, d16);
        const int32_t* const spos = v.ppos1 + mcf_pair_index(0, sbit, d4);
        const int32_t* const src = v.order[0] + mcf_pair_index(0, cx.cur, d4);
        int32_t* const dst = v.order[0] + mcf_pair_index(0, nbit, d4);
        int32_t* const pnext = v.posbuf[0] + mcf_pair_index(0, nbit, d4);
        if (catch0) ndc = src[jc];
        for (int32_t j = lo + threadIdx.x; j < hi; j += THREADS) mcf_apply_one_paths_at(v, cx, srec, spos, src, dst, pnext, j);
        if (catch0) mcf_apply_catch_up_store_at(dst, pnext, jc, ndc);
        for (int32_t j = jc + (kCatchUpBeside ? THREADS : 0); j < phi; j += THREADS)
            if (j < lo || j >= hi) mcf_apply_one_paths_at(v, cx, srec, spos, src, dst, pnext, j);
    } else {
        const McfNode* const srec = cx.pv_result == 1 ? v.rec1 : v.rec2;
        const int32_t* const spos = cx.pv_result == 1 ? v.ppos1 : v.ppos2;
        if (catch0) ndc = (cx.cur ? v.order[1] : v.order[0])[jc];
        for (int32_t j = lo + threadIdx.x; j < hi; j += THREADS) mcf_apply_one_paths(v, cx, srec, spos, j);
        if (catch0) mcf_apply_catch_up_store(v, cx, jc, ndc);
        for (int32_t j = jc + (kCatchUpBeside ? THREADS : 0); j < phi; j += THREADS)
            if (j < lo || j >= hi) mcf_apply_one_paths(v, cx, srec, spos, j);
    }
}

// ---- at the budget: is any arc still eligible?  (simplex.py:1678-1699; saves the host a pricing pass + three syncs)
// Three barriers inside, taken by every lane or by none (the status is the LDS image's).
template <int THREADS> __device__ __forceinline__ void small_budget_check(const McfView& v, const McfView& g, McfCtx* c, int& s_any) {
    if (c->status == MCF_PIVOT_LIMIT && !c->limit_checked) {
        if (threadIdx.x == 0) s_any = 0;
        __syncthreads();
        int any = 0;
        for (int64_t i = threadIdx.x; i < g.m && !any; i += THREADS)
            if (v.state[i] && mcf_violation(v, i) > 0) any = 1;
        if (any) s_any = 1;
        __syncthreads();
        if (threadIdx.x == 0) { if (s_any) c->limit_checked = 1; else c->status = MCF_OPTIMAL; }
        __syncthreads();
    }
}

// The whole solve of one LDS-resident instance by one workgroup of THREADS lanes (k_solve_small: one instance per launch;
// k_solve_small_batch: one instance per workgroup of the launch)
// FRONT: the kernel of a Dantzig solve with the plain key whose reduced costs fit 32 bits (small_front_for on the host) -- the
// narrow register sweep, the arg-max that hands the winner over, begin in one round trip; rule, sweep and key width are
// compile-time constants there.  !FRONT: every other rule, key mode and range, with 64-bit keys.  Two kernels, not one kernel
// with a per-launch switch: with both fronts in one loop the 64-bit path, Devex and the candidate list all lost 2 - 5 %
// (profiles/small_loop_front_stamps.txt).
// ---- control in registers.  Every wave carries the control block itself -- a private McfCtx whose fields live in scalar
// registers -- and takes every scalar decision of a pivot itself, from broadcast LDS reads: mcf_pivot_begin_t,
// mcf_pivot_decide, mcf_pivot_finish and mcf_apply_one run on that private copy (v.ctx points to it), the very functions
// of the other paths.  Nothing goes through an LDS mailbox, no wave waits for lane 0, and the barriers that only ordered
// "lane 0 wrote, everybody reads" are gone.  The LDS image is written once after the loop.
// THE RULE that replaces those barriers: between two barriers no wave reads an LDS location that a faster wave can write
// before the next barrier.  Its instances here:
//   * the parallel search's residual / by-depth scratch has LDS of its own, not the segment table's (the general finish pass
//     fills that table; the one that runs here leaves it alone);
//   * finish and apply run between the SAME two barriers, the finish pass in the last wave (mcf_pivot_finish_t<true>), the
//     apply pass in every wave (mcf_apply_one_paths), and touch disjoint LDS words.  Finish reads the recorded paths (path /
//     rec / ppos, ordered by the search barrier) and the descriptor in registers; it writes arcw[].flow, state[], the Devex
//     weights, node[].size along both sides and node[stem[i]].{parent, pred, size} -- never a depth word, never the segment
//     table.  Apply reads order[cur] and the same recorded paths (its sources come from them: mcf_apply_source_paths); it
//     reads and writes pi[] and node[].depth and writes order[cur ^ 1] and pos[cur ^ 1].  A wave that still runs its ratio
//     tests or decides reads the residual scratch, the per-wave counts and the recorded paths: nothing either pass writes.
//     The end-of-iteration barrier orders both passes' stores before the next sweep, begin and search;
//   * inside the apply pass the catch-up range's read of order[cur] is issued in front of the first loop (small_apply): nobody
//     writes order[cur] between these two barriers, and the catch-up's stores go to other positions of order[cur ^ 1] and other
//     nodes of pos[cur ^ 1] than the first loop's;
//   * the end points' records and positions (r0u / r0w / p0u / p0w) are begin's reads, taken before the search barrier:
//     the finish pass rewrites node[u_in];
//   * begin reads arcw[e].flow and state[e], finish writes them: all of begin's reads precede the search barrier;
//   * an iteration that pivots on nothing (empty Devex block, exhausted list, budget, optimal) takes one barrier before
//     it continues: the next iteration rewrites the per-wave arg-max slots and the candidate list;
//   * the front kernel's per-wave slots (key + the winner's record) are written before the arg-max barrier, read right
//     behind it by every wave, and rewritten only by the next iteration's arg-max: the apply barrier, or the barrier of an
//     iteration that pivots on nothing, lies between.
// Rule-specific bookkeeping in memory -- the entering arc's Devex weight and the list of touched weights -- is stored by
// mcf_pivot_decide with the same value from every lane; nothing reads it before the next barrier.  A tuner step
// (block_granules / num_blocks) is computed in every wave alike.
// Every __shared__ variable of the loop is declared here and handed to the stages: the LDS offsets are this function's.
template <int THREADS, bool FRONT>
__device__ __forceinline__ void solve_small_body(const McfView& g, const SmallLayout& L, int32_t rule_in,
                                                 McfCand* __restrict__ list, int64_t cap, char* smem, McfCtx* host_ctx) {
    static_assert(THREADS == 256 || THREADS == 1024, "the two widths the loop is tuned and instantiated for");
    const int32_t rule = FRONT ? (int32_t)MCF_RULE_DANTZIG : rule_in;
#ifdef MCF_STAMPS
    unsigned long long stamps_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last_ = __builtin_amdgcn_s_memtime();
    unsigned long long last_wave_ = 0;
    if (threadIdx.x == 0) { for (int i = 0; i < 24; ++i) mcf_stamp_acc[i] = 0; mcf_stamp_last = last_; }
#ifdef MCF_WAVE_STAMPS
    if (threadIdx.x < 16 * 6) (&mcf_wave_acc[0][0])[threadIdx.x] = 0;
#endif
#endif
    const SmallSizes sizes = small_sizes(g);
    McfView v = small_map_view<FRONT>(g, L, smem);
    small_copy_image<THREADS, true>(g, L, smem, v.weight != nullptr, sizes);
    __syncthreads();
    STAMP(0);

    McfCtx* const c = v.ctx;   // the LDS image of the control block: read once below, written once after the loop
    if (threadIdx.x == 0) arm_ctx(c, cap);  // (what k_ctl does for the other paths; visible after the barrier below)
    __shared__ int32_t s_gran[MCF_NUM_BUCKETS][MCF_GRANULES + 1];
    const bool devex = !FRONT && rule == MCF_RULE_DEVEX_BLOCK && g.dx;
    small_load_granules<THREADS>(g, devex, s_gran);
    // candidate-list rule: the list is the best arc of each head bucket (= of each of the 8 pricing
    // workgroups the three-kernel path would use at this size); minor iterations re-price just
    // those 8 arcs.  The list survives between launches in `list` (global).
    const bool listing = !FRONT && rule == MCF_RULE_CANDIDATE_LIST;
    __shared__ int64_t s_lk[MCF_NUM_BUCKETS], s_la[MCF_NUM_BUCKETS];
    if (listing && threadIdx.x < MCF_NUM_BUCKETS) { s_lk[threadIdx.x] = list[threadIdx.x].key; s_la[threadIdx.x] = list[threadIdx.x].arc; }
    __syncthreads();   // arm_ctx, the granule table and the list -> every lane's reads below and in the loop
    __shared__ int32_t s_gsum[MCF_GRANULES + 1];
    small_sum_granules(devex, s_gran, s_gsum);
    __syncthreads();   // the sums -> every wave's reads (once here, and per sweep under Devex)
    constexpr bool kScalar = small_scalar_control(THREADS);
    const int64_t priced_all = uni32<kScalar>(s_gsum[MCF_GRANULES] - s_gsum[0]);

    // ---- lane map of the sweep: THREADS / 8 lanes per head bucket, all eight buckets at once
    constexpr int kPer = THREADS / MCF_NUM_BUCKETS;
    constexpr int kReg = small_reg_arcs(THREADS);
    static_assert(kPer == 32 || kPer % 64 == 0, "a head bucket's lanes are half a wave or whole waves");
    const int px = threadIdx.x / kPer, pl = threadIdx.x % kPer;
    const int sweep = FRONT ? (int)kSweepPlain
                            : (devex ? kSweepDevex : (rule != MCF_RULE_DEVEX_BLOCK && v.key_mode == MCF_KEY_PLAIN ? kSweepPlain : kSweepGeneric));
    // Plain sweep: the arcs a lane prices are the same at every pivot (whole buckets), and tail / head / cost / orig never
    // change during a launch: the first kReg of them live in registers from here on.  (Slots past the lane's last arc price
    // arc 0 with its state masked to 0.)
    int32_t r_tail[kReg], r_head[kReg], r_cost[kReg], r_orig[kReg];
    uint32_t r_info[kReg];   // (small_info: what the arg-max hands over to begin)
    int32_t r_n = 0;   // slots in use
    // The front kernels: the even deal over all arcs (a compile-time constant); the general ones: per head bucket.
    // r_step apart either way, and slot q of a lane is engine arc r_lo + q * r_step.
    constexpr int kRegFew = small_reg_arcs_few(THREADS, FRONT);
    static_assert(kRegFew <= kReg, "the shorter unrolled sweep is a prefix of the longer");
    const bool even = FRONT && sweep == kSweepPlain && rule == MCF_RULE_DANTZIG;
    const int32_t r_step = even ? THREADS : kPer;
    const int32_t r_lo = even ? mcf_even_arc(s_gran[0][0], (int32_t)threadIdx.x, 0, THREADS) : s_gran[px][0] + pl;
    const int32_t r_hi = even ? s_gran[MCF_NUM_BUCKETS - 1][MCF_GRANULES] : s_gran[px][MCF_GRANULES];
    const bool r_few = even && uni32<kScalar>(mcf_even_reg_slots(s_gran[MCF_NUM_BUCKETS - 1][MCF_GRANULES] - s_gran[0][0], THREADS, kRegFew, kReg)) == kRegFew;
#pragma unroll
    for (int k = 0; k < kReg; ++k) {
        const int32_t i = r_lo + k * r_step;
        const bool on = sweep == kSweepPlain && i < r_hi;
        r_tail[k] = on ? v.tail[i] : 0; r_head[k] = on ? v.head[i] : 0; r_cost[k] = on ? v.cost[i] : 0; r_orig[k] = on ? v.orig[i] : 0;
        r_info[k] = small_info(r_tail[k], r_head[k], k);
        r_n += on ? 1 : 0;
    }
    // (small_price_flat) a slot's packed key as a register pair of its own: ~id below, this sweep's violation above it -- the
    // 64-bit compare reads the pair as it stands, where a key built per sweep costs an OR and a copy per slot
    // (only there: every other kernel declares one dead element and compiles to what it was)
    typedef uint32_t small_u32x2 __attribute__((ext_vector_type(2)));
    small_u32x2 r_key[small_price_flat(THREADS, FRONT) ? kReg : 1];
    if constexpr (small_price_flat(THREADS, FRONT)) {
#pragma unroll
        for (int k = 0; k < kReg; ++k) { r_key[k].x = (uint32_t)~r_orig[k]; r_key[k].y = 0; }
    }
    // The front (compile-time): 32-bit keys on the plain register sweep, and with them the arg-max that hands the winner's
    // record to begin.  64-bit keys price from registers or LDS, reduce with block_argmax_all and let begin look the arc up.
    const bool reg_plain = sweep == kSweepPlain;
    constexpr bool nar = FRONT;
    constexpr bool kDescOnce = small_desc_once(THREADS, FRONT);
    constexpr bool kDecideFlat = small_decide_flat(THREADS, FRONT);
    constexpr bool kPriceFlat = small_price_flat(THREADS, FRONT);
    constexpr bool kPairs = small_pair_arith(THREADS, FRONT);
    constexpr int kPriceChains = small_price_chains(THREADS, FRONT);
    constexpr bool hand = FRONT;
    const int32_t* const pi32 = reinterpret_cast<const int32_t*>(v.pi);   // low words of the potentials
    // ---- control in registers (see above): a private copy of the control block in every wave
    McfCtx cx = *c;            // (broadcast reads; the fields the loop never touches are dead after this)
    small_ctx_uniform<kScalar>(cx);
    cx.max_pivots = uni64<kScalar>(cx.max_pivots); cx.minor_cap = uni32<kScalar>(cx.minor_cap); cx.auto_tune = uni32<kScalar>(cx.auto_tune);
    cx.devex_cyclic = uni32<kScalar>(cx.devex_cyclic); cx.max_granules = uni32<kScalar>(cx.max_granules);
    v.ctx = &cx;
    const int64_t adj2 = uni64<kScalar>(cx.pv_adj[2]), adj3 = uni64<kScalar>(cx.pv_adj[3]);   // (never fetched on this path: whatever the image holds)
    int64_t* const scratch = reinterpret_cast<int64_t*>(smem + L.scratch);
    __shared__ McfCycle s_cy;   // the two-lane climb's result (the rare path: shallow end points, trees above kSmallCycleMaxNodes)
    __shared__ int s_ok;
    __shared__ SmallCycleAcc s_acc;
    __shared__ SmallWaveSlot s_slot[THREADS / 64];               // the handing-over arg-max's per-wave slots (front kernels)
    for (;;) {
        if (cx.status != MCF_RUNNING) break;   // (uniform: every wave leaves together)
#if defined(MCF_STAMPS) && defined(MCF_WAVE_STAMPS)
        if ((cx.pivots & 15) == 0) { MCF_WAVE_PROBE(&s_acc.c[0][0]); if (threadIdx.x == 64) mcf_wave_acc[1][5] += 1; }   // (the probe delays wave 0: one pivot in 16)
#endif
        MCF_WAVE_T0();
        const bool minor = listing && cx.minor_left > 0;
        int32_t bg0, bg1;
        devex_block_granules(cx, devex, bg0, bg1);
        // ---- price: the arc set of k_price for shard 0 of 1
        int64_t key = 0, arc = -1;
        McfCandX wx;   // the winner's record (hand)
        wx.rc = 0; wx.arc = -1; wx.tail = 0; wx.head = 0; wx.state = 0; wx.pad = 0;
        uint64_t nbest = 0xffffffffull;   // narrow: (violation << 32) | ~orig of the lane's best; high word 0: nothing eligible
        uint32_t info = 0;                // ... and its end points, slot and state (small_info)
        if (!minor) {
            if (nar) {
                // 32-bit keys: the low words of the potentials, one compare and two selects per arc.  The plain maximum of
                // (violation << 32) | ~orig is mcf_cand_better's winner -- larger violation, then lower id -- and never ties.
                // The first NS register slots; under the even deal NS = kRegFew when those hold every arc (r_few, uniform).
                auto slots = [&](auto ns) {
                    constexpr int NS = decltype(ns)::value;
                    int32_t st[NS], pt[NS], ph[NS];
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        st[k] = v.state[k < r_n ? r_lo + k * r_step : 0];
                        pt[k] = pi32[2 * r_tail[k]];
                        ph[k] = pi32[2 * r_head[k]];
                    }
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        const int32_t rc = (int32_t)((uint32_t)r_cost[k] + (uint32_t)pt[k] - (uint32_t)ph[k]);
                        const int32_t s = k < r_n ? st[k] : 0;
                        const int32_t viol = s > 0 ? -rc : rc;
                        const uint64_t p = ((uint64_t)(uint32_t)((s != 0 && viol > 0) ? viol : 0) << 32) | (uint32_t)~r_orig[k];
                        if (p > nbest) { nbest = p; info = r_info[k] | ((uint32_t)s & 0x80000000u); }
                    }
                };
                // The same sweep counted in issue slots (kPriceFlat): the violation without a compare (mcf_narrow_violation_signed),
                // keys compared as signed 64-bit numbers so that nothing is clamped, and kPriceChains accumulators over alternate
                // slots merged by the same compare -- one chain's compare has the other's work behind it instead of a wait for VCC.
                // A slot past the lane's last arc holds cost 0, tail = head = 0 and id 0: reduced cost 0 whatever state it reads,
                // its key is the start value and replaces nothing -- no mask.
                auto slots_flat = [&](auto ns) {
                    constexpr int NS = decltype(ns)::value;
                    int32_t st[NS], pt[NS], ph[NS];
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        st[k] = v.state[k < r_n ? r_lo + k * r_step : 0];
                        pt[k] = pi32[2 * r_tail[k]];
                        ph[k] = pi32[2 * r_head[k]];
                    }
                    int64_t nb[kPriceChains];
                    uint32_t inf[kPriceChains];
                    // (a chain starts from its first slot's key, eligible or not, and the start value is compared once, behind the
                    //  merge: every ineligible key is <= mcf_narrow_start() < every eligible one)
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        const int32_t rc = (int32_t)((uint32_t)r_cost[k] + (uint32_t)pt[k] - (uint32_t)ph[k]);
                        // mcf_narrow_key(violation, id) assembled in place: the low word never changes, the high one is written here
                        r_key[k].y = (uint32_t)mcf_narrow_violation_signed(st[k], rc);
                        const int64_t p = __builtin_bit_cast(int64_t, r_key[k]);
                        const int a = k % kPriceChains;
                        if (k < kPriceChains || p > nb[a]) { nb[a] = p; inf[a] = r_info[k] | ((uint32_t)st[k] & 0x80000000u); }
                    }
#pragma unroll
                    for (int a = 1; a < kPriceChains; ++a) if (nb[a] > nb[0]) { nb[0] = nb[a]; inf[0] = inf[a]; }
                    if (!(nb[0] > mcf_narrow_start())) { nb[0] = mcf_narrow_start(); inf[0] = 0; }
                    nbest = (uint64_t)nb[0]; info = inf[0];   // (high word >= 0: the start value's or an eligible arc's)
                };
                if constexpr (kPriceFlat) {
                    if (r_few) slots_flat(SmallSlots<kRegFew>{});
                    else slots_flat(SmallSlots<kReg>{});
                } else {
                    if (r_few) slots(SmallSlots<kRegFew>{});
                    else slots(SmallSlots<kReg>{});
                }
                int32_t q = kReg;   // (no trip when r_few)
                for (int32_t i = r_lo + kReg * r_step; i < r_hi; i += r_step, ++q) small_price_lds_narrow(v, i, q, nbest, info);
                // the present form, for the candidate list's entries and for the record
                if (nbest >> 32) { key = (int64_t)(nbest >> 32); arc = mcf_pack_arc((int32_t)~(uint32_t)nbest, r_lo + (int32_t)((info >> 22) & 0x1ff) * r_step); }
            } else if (reg_plain) {
                // one LDS round trip for the whole lane: states and potentials of all its register arcs, then selects
                auto slots = [&](auto ns) {
                    constexpr int NS = decltype(ns)::value;
                    int32_t st[NS];
                    int64_t pt[NS], ph[NS];
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        st[k] = v.state[k < r_n ? r_lo + k * r_step : 0];
                        pt[k] = v.pi[r_tail[k]];
                        ph[k] = v.pi[r_head[k]];
                    }
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        const int64_t rc = (int64_t)r_cost[k] + pt[k] - ph[k];
                        const int32_t s = k < r_n ? st[k] : 0;
                        const int64_t viol = s > 0 ? -rc : rc;
                        const int64_t pid = mcf_pack_arc(r_orig[k], r_lo + k * r_step);
                        if (s != 0 && viol > 0 && mcf_cand_better(viol, pid, key, arc)) { key = viol; arc = pid; }
                    }
                };
                if (r_few) slots(SmallSlots<kRegFew>{});
                else slots(SmallSlots<kReg>{});
                for (int32_t i = r_lo + kReg * r_step; i < r_hi; i += r_step) small_price_lds<kSweepPlain>(v, rule, devex, i, key, arc);
            } else {
                const int32_t lo = s_gran[px][bg0], hi = s_gran[px][bg1];
                if (sweep == kSweepDevex) for (int32_t i = lo + pl; i < hi; i += kPer) small_price_lds<kSweepDevex>(v, rule, devex, i, key, arc);
                else if (sweep == kSweepPlain) for (int32_t i = lo + pl; i < hi; i += kPer) small_price_lds<kSweepPlain>(v, rule, devex, i, key, arc);
                else for (int32_t i = lo + pl; i < hi; i += kPer) small_price_lds<kSweepGeneric>(v, rule, devex, i, key, arc);
            }
        }
        STAMP(1);
        // ---- arg-max: (key, arc) uniform in every wave afterwards
        if (listing) {
            if (!minor) {
                if constexpr (kPer >= 64) {   // the list: each head bucket's best
                    constexpr int kWpb = kPer / 64;   // waves per bucket
                    __shared__ int64_t s_wk[THREADS / 64], s_wa[THREADS / 64];
                    wave_argmax(key, arc);
                    if ((threadIdx.x & 63) == 0) { s_wk[threadIdx.x >> 6] = key; s_wa[threadIdx.x >> 6] = arc; }
                    __syncthreads();   // per-wave candidates -> the bucket's lane
                    if (threadIdx.x < MCF_NUM_BUCKETS) {
                        const int w = kWpb * threadIdx.x;
                        int64_t bk = s_wk[w], ba = s_wa[w];
                        for (int q = 1; q < kWpb; ++q)
                            if (mcf_cand_better(s_wk[w + q], s_wa[w + q], bk, ba)) { bk = s_wk[w + q]; ba = s_wa[w + q]; }
                        s_lk[threadIdx.x] = bk; s_la[threadIdx.x] = ba;
                    }
                } else {
                    half_wave_argmax(key, arc);
                    if (pl == 0) { s_lk[px] = key; s_la[px] = arc; }
                }
                __syncthreads();   // the new list -> every wave's arg-max over it
            }
            // lanes 0-7 of every wave take one listed arc each (a minor iteration re-prices it), the wave reduces:
            // mcf_cand_better is a total order, so the winner is the one the lane-by-lane scan found
            const int32_t l = (int32_t)(threadIdx.x & 63);
            key = 0; arc = -1;
            if (l < MCF_NUM_BUCKETS) {
                arc = s_la[l];
                key = minor ? mcf_minor_key(v, arc) : s_lk[l];
                if (key <= 0) { key = 0; arc = -1; }
            }
            wave_argmax(key, arc);
        } else if constexpr (FRONT) {
            small_handover_publish(nbest, arc, info, s_slot);
            __syncthreads();   // per-wave slots -> every wave's pick
            small_handover_pick<THREADS>(s_slot, key, arc, wx);
        } else {
            block_argmax_all<THREADS>(key, arc);
        }
        STAMP(2);
        MCF_SLOT_PROBE_HERE();
        // ---- pivot: every wave decides, everything it touches is in LDS or in its registers
        if (cx.pivots < cx.max_pivots)
            cx.arcs_priced += minor ? (int64_t)MCF_NUM_BUCKETS : (devex ? (int64_t)uni32<kScalar>(s_gsum[bg1] - s_gsum[bg0]) : priced_all);
        MCF_PSTAMP(12);
        // begin: with the winner's record in registers (wx), the arc's capacity and flow and its end points' records and
        // positions all hang on values known here -- one broadcast round trip; without it the arc's record first, then its end
        // points' records, positions and potentials -- two.  The records the decision will need are fetched here (WITH_CY).
        McfCycle cy;
        bool go;
        if constexpr (hand) go = mcf_pivot_begin_t<true>(v, key, arc, rule, &wx, &cy);
        else go = mcf_pivot_begin_t<true>(v, key, arc, rule, nullptr, &cy);
        small_ctx_uniform<kScalar>(cx);
        MCF_PSTAMP(13);
        if (!go) {   // nothing to pivot on: uniform, every wave takes this way
            STAMP(3);
            __syncthreads();   // this iteration's reads of the per-wave arg-max slots and of the list -> the next one's writes
            STAMP(5);
            continue;
        }
        small_cycle_ends<kScalar>(cy);
        const int32_t deep = cy.r0u.depth > cy.r0w.depth ? cy.r0u.depth : cy.r0w.depth;
        // Cycle search: every lane takes nodes (small_cycle_parallel) while the tree is small enough; else lanes 0 and 1 climb
        // one side each (pivot_climb_2lanes) and every wave reads their result.
        // (end points that hang close to the root -- the first pivots of a cold start -- are climbed: a level or two of
        //  LDS round trips beat the parallel search's fixed cost: 144 K vs 126 K pivots/s over the first 25 pivots)
        if (v.n_nodes <= kSmallCycleMaxNodes && deep > 3) {
            small_cycle_parallel<THREADS, FRONT>(v, s_acc, scratch, cy);   // (one barrier inside)
            MCF_PSTAMP(15);
            if constexpr (kDecideFlat && kPairs) mcf_pivot_decide_flat_t<true>(v, mcf_view_paths(v), cy, mcf_pair_dist4(v.n_nodes), mcf_pair_dist16(v.n_nodes));
            else if constexpr (kDecideFlat) mcf_pivot_decide_flat(v, mcf_view_paths(v), cy);
            else mcf_pivot_decide(v, mcf_view_paths(v), cy);
        } else {
            if (threadIdx.x < 2) {
                const bool ok = pivot_climb_2lanes(v, &s_cy);
                if (threadIdx.x == 0) s_ok = ok ? 1 : 0;
            }
            __syncthreads();   // the climbed paths, s_cy and s_ok -> every wave's decision and the finish pass
            if (uni32<kScalar>(s_ok)) {
                cy = s_cy;
                uni_cycle<kScalar>(cy);
                mcf_pivot_decide(v, mcf_view_paths(v), cy);
            } else {
                cx.status = MCF_INTERNAL_ERROR;
            }
        }
        small_ctx_uniform<kScalar>(cx);
        if constexpr (!kDescOnce) { if (threadIdx.x == 0) small_desc_store(c, cx, adj2, adj3); }
        MCF_PSTAMP(16);
        STAMP(3);
        MCF_WAVE_STAMP(2);
        // (no barrier: the finish pass reads the recorded paths, which the search barrier ordered, and the descriptor in registers)
        // finish and apply between the same two barriers: the LAST wave alone finishes (uniform per wave; the pass needs
        // n1 + n2 and k + 1 lanes, about ten on netgen_8_08a) while the others apply; it then takes the apply positions from
        // lo + THREADS - 64 on, which most pivots do not have.  See THE RULE above for why the two never meet.
        if ((int32_t)threadIdx.x >= THREADS - 64) {
            MCF_LAST_WAVE_BEGIN();
            if constexpr (kPairs) mcf_pivot_finish_pairs<small_finish_one_trip(THREADS, FRONT)>(v, mcf_view_paths(v), mcf_pair_dist4(v.n_nodes), mcf_pair_dist16(v.n_nodes), (int32_t)threadIdx.x - (THREADS - 64), 64);
            else mcf_pivot_finish_t<true>(v, mcf_view_paths(v), (int32_t)threadIdx.x - (THREADS - 64), 64);
            MCF_LAST_WAVE_STAMP();
            MCF_WAVE_STAMP(4);
        }
        STAMP(4);
        small_apply<THREADS, FRONT>(v, cx);
        MCF_WAVE_STAMP(3);
        __syncthreads();   // the apply pass's order / position / potential / depth stores and the finish pass's flows and states
                           // -> the next iteration's sweep, begin and search
        cx.apply = 0;
        STAMP(5);
    }
    // the control state goes back into the LDS image, once
    if (threadIdx.x == 0) {
        small_ctx_store(c, cx);
        if constexpr (kDescOnce) small_desc_store_all(c, cx);
    }
    v.ctx = c;
    __syncthreads();   // the LDS control block -> the budget check and the copy-out
    __shared__ int s_any;
    small_budget_check<THREADS>(v, g, c, s_any);   // (three barriers inside, when at the budget)
    small_copy_image<THREADS, false>(g, L, smem, v.weight != nullptr, sizes);
    // ... and straight into the host's pinned copy: the host then only waits for the stream, no read-back copy
    if (host_ctx) copy_words<THREADS>(host_ctx, smem + L.ctx, (uint32_t)sizeof(McfCtx));
    if (listing && threadIdx.x < MCF_NUM_BUCKETS) list[threadIdx.x] = McfCand{s_lk[threadIdx.x], s_la[threadIdx.x]};
#ifdef MCF_STAMPS
    STAMP(6);
    if (threadIdx.x == 0) {  // diagnostic build only: cycle sums into the (global) path scratch, read by mcf_debug_stamps
        unsigned long long* out = reinterpret_cast<unsigned long long*>(g.rec1);
        for (int i = 0; i < 7; ++i) out[i] = stamps_[i];
        for (int i = 0; i < 24; ++i) g_pivot_stamps[i] += mcf_stamp_acc[i];
    }
    if (threadIdx.x == THREADS - 64) reinterpret_cast<unsigned long long*>(g.rec1)[7] = last_wave_;   // (0 when nothing ran beside)
#ifdef MCF_WAVE_STAMPS
    if (threadIdx.x < 16 * 6 && (int64_t)g.n_nodes * (int64_t)sizeof(McfNode) >= (8 + 16 * 6) * 8)   // (only where the path scratch holds them)
        reinterpret_cast<unsigned long long*>(g.rec1)[8 + threadIdx.x] = (&mcf_wave_acc[0][0])[threadIdx.x];
#endif
#endif
}

// (waves per SIMD stated: one workgroup per CU -- the LDS image allows no second -- so 256 lanes are ONE wave per SIMD and may
//  use its whole register file; left to guess, the compiler kept room for two and put 20 B per lane into scratch)
template <int THREADS, bool FRONT>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(THREADS / 256, THREADS / 256))) void k_solve_small(McfView g, SmallLayout L, int32_t rule,
                                                          McfCand* __restrict__ list, int64_t cap, McfCtx* host_ctx) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    solve_small_body<THREADS, FRONT>(g, L, rule, list, cap, smem, host_ctx);
}

// Many independent small instances side by side: workgroup b solves jobs[b] from start to finish in its own CU's LDS.
// Nothing is shared between the workgroups, so a batch of >= 256 instances keeps every CU of the chip busy with
// latency-bound work that a single instance can only ever give one CU of (mcf_solve_batch).
struct SmallJob {
    McfView g;
    SmallLayout L;
    int32_t rule;
    int32_t narrow;     // the job's reduced costs fit 32 bits (small_narrow_for); the host sorts the jobs by front (small_front_for)
    McfCand* list;
    int64_t cap;
    McfCtx* host_ctx;   // pinned: the final control block goes straight to the host
};

template <int THREADS, bool FRONT>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(THREADS / 256, THREADS / 256))) void k_solve_small_batch(const SmallJob* __restrict__ jobs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SmallJob& J = jobs[blockIdx.x];   // uniform per workgroup: scalar loads
    solve_small_body<THREADS, FRONT>(J.g, J.L, J.rule, J.list, J.cap, smem, J.host_ctx);
}

// ------------------------------------------------------------------ k_ctl: (re)arm the control block
__global__ void k_ctl(McfCtx* c, int64_t max_pivots, int resume) {
    c->max_pivots = max_pivots;
    c->limit_checked = 0;
    if (resume && c->status == MCF_PIVOT_LIMIT && c->pivots < max_pivots) c->status = MCF_RUNNING;
}

__global__ void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}

// ------------------------------------------------------------------ k_fork: the device copy of mcf_fork / mcf_restore
// One launch writes every state array of every destination handle: a grid-stride loop over (chunk, destination group)
// items (mcf_core.h: mcf_fork_*).  A chunk is read once -- 16 bytes per lane, the last bytes % 16 of a segment one byte per
// lane -- and stored from registers to up to MCF_FORK_GROUP destinations, so that `count` forks read the source about
// count / MCF_FORK_GROUP times (from L2 after the first) instead of count times.  NT: non-temporal stores, for copies larger
// than the Infinity Cache, whose lines nobody reads again before they are evicted (chosen by size, MCF_FORK_NT = 0 / 1 forces;
// measured: profiles/fork_scenarios.txt).
typedef unsigned int fork_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ __launch_bounds__(MCF_FORK_THREADS) void k_fork(const McfForkSeg* __restrict__ seg, int32_t nseg, int64_t total_chunks,
                                                           char* const* __restrict__ dst_table, int64_t count) {
    const int64_t items = mcf_fork_items(total_chunks, count);
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        int64_t chunk, d_lo, d_hi;
        mcf_fork_item(item, total_chunks, count, &chunk, &d_lo, &d_hi);
        const int32_t si = mcf_fork_find(seg, nseg, chunk);   // (uniform per workgroup)
        const McfForkSeg sg = seg[si];
        int64_t vec, tail;
        mcf_fork_lane(sg.bytes, chunk - sg.chunk0, (int32_t)threadIdx.x, &vec, &tail);
        if (vec >= 0) {
            const fork_u32x4 x = *reinterpret_cast<const fork_u32x4*>(sg.src + vec);
            for (int64_t d = d_lo; d < d_hi; ++d) {
                fork_u32x4* q = reinterpret_cast<fork_u32x4*>(dst_table[d * nseg + sg.slot] + vec);
                if (NT) __builtin_nontemporal_store(x, q); else *q = x;
            }
        }
        if (tail >= 0) {
            const char x = sg.src[tail];
            for (int64_t d = d_lo; d < d_hi; ++d) dst_table[d * nseg + sg.slot][tail] = x;
        }
    }
}

#include "mcf_passes_dev.h"

}  // namespace

// ====================================================================== handle
struct mcf_handle {
    McfHostImage im;
    mcf_options opt{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool stream_owned = true;   // false: borrowed from the per-device pool (small / mid-size instances)
    // device arrays
    int32_t *d_tail = nullptr, *d_head = nullptr, *d_cost = nullptr, *d_orig = nullptr;
    int8_t* d_state = nullptr;
    int8_t* d_prio = nullptr;    // MCF_KEY_PRIORITY: per-arc preference bits, engine order
    float* d_weight = nullptr;
    McfArcW* d_arcw = nullptr;
    int64_t* d_pi = nullptr;
    McfNode* d_node = nullptr;
    int32_t *d_order0 = nullptr, *d_order1 = nullptr, *d_path1 = nullptr, *d_path2 = nullptr, *d_ppos1 = nullptr, *d_ppos2 = nullptr;
    McfNode *d_rec1 = nullptr, *d_rec2 = nullptr;
    int64_t *d_rcache = nullptr, *d_adj_off = nullptr, *d_adj = nullptr;
    int32_t* d_vkey = nullptr;   // compressed Dantzig keys (4 B per arc), see McfView::vkey
    bool nt_sweep = false;       // the key-code sweep is larger than the Infinity Cache: non-temporal loads
    int32_t *d_pos0 = nullptr, *d_pos1 = nullptr, *d_psz0 = nullptr, *d_psz1 = nullptr;
    int32_t *d_reach = nullptr, *d_chg = nullptr;  // coarse index over the position-space sizes + its scratch
    // blocked preorder list (large trees): d_order0/1 and d_psz0/1 are then the two slot arenas, d_pos0 is loc[]
    bool bpl = false;
    int bpl_shift = 0, bpl_cap = 0, bpl_dense = 0, bpl_grid = 1;
    McfBlkMeta* d_bmeta[2] = {nullptr, nullptr};
    int32_t* d_bext[2] = {nullptr, nullptr};
    McfDirty* d_dirty = nullptr;
    int64_t* d_swept = nullptr;  // arcs swept per pricing workgroup (summed by mcf_get_result)
    McfDevex* d_dx = nullptr;        // Devex: granule table + touched-weight list
    int32_t* d_full_tab = nullptr;   // sharded full sweeps: (lo, hi) of this rank's share of bucket x, [8][2]
    bool rcached = false;     // large instance: resident reduced costs + k_rcupd
    int rcupd_blocks = 1;
    McfSeg* d_seg = nullptr;
    McfCtx* d_ctx = nullptr;
    McfCand* d_cand = nullptr;
    McfCandX* d_candx = nullptr;    // candidate cache (candidate-list rule, single GPU, grid path)
    McfCand* d_cand_aux = nullptr;  // scratch for mcf_price_once / mcf_time_pricing: the live list in d_cand must survive them
    McfCand* d_one = nullptr;
    McfCtx* h_ctx = nullptr;   // pinned
    McfCand* h_one = nullptr;  // pinned
    McfView view{};
    // Every device array of the solver state, recorded by the one place that allocates them (alloc_wire); mcf_add_arcs keeps the
    // lengths current.  mcf_fork / mcf_restore copy the `state` ones and compare the lengths; the others are scratch that every
    // pivot writes before it reads.
    struct DevArray { void** field; size_t bytes; bool state; const char* name; };
    std::vector<DevArray> arrays;
    bool scan_ok = false, want_vkey = false, want_dirty = false, want_candx = false;   // what decide_geometry chose
    bool rc_partial = false;
    int32_t key_mode = 0;        // McfView::key_mode as decided from the options
    // what mcf_restore compares: every value that decides which arrays exist and how long they are (shape_of; the array
    // lengths themselves are compared from `arrays`)
    std::vector<std::pair<const char*, int64_t>> shape;
    bool dx_filled = false;      // the Devex granule table was uploaded (once)
    int price_blocks = 1;
    int apply_blocks = 1;
    int32_t climb_budget = INT32_MAX;  // round trips the cycle climb may take before the scan takes over
    bool small = false;       // whole instance fits in LDS: fused single-workgroup pivot loop
    int small_threads = 0;    // ... and the width of that workgroup (small_threads_for at mcf_create)
    bool small_narrow_ok = true;   // MCF_SMALL_NARROW as read at mcf_create (small_narrow_allowed)
    bool mid = false;         // mid-size instance: persistent single-workgroup pivot loop over global memory (k_solve_mid)
    SmallLayout small_layout{};
    int64_t shard = 0, shards = 1;
    int64_t shard_arcs = 0;  // arcs of this rank's shard (all buckets)
    int64_t priced_per_pass = 0;
    // graph
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_batch = 0;
    // overlapped graphs: pricing of pivot t+1 runs beside the tree permutation of pivot t (needs only the reduced-cost half)
    bool overlap = false;
    bool overlap_cfg = false;   // what mcf_create decided (dropping the reduced costs turns it off until the next reset)
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> fork_ev;   // two per slot: pivot done (main -> side), priced (side -> main)
    // profiling events
    std::vector<hipEvent_t> events;
    hipEvent_t loop_ev[2] = {nullptr, nullptr};  // around every launch of a persistent pivot loop
    // bookkeeping
    mcf_stats stats{};
    int64_t total_cap = 0;
    std::string err;
    bool solved_once = false;
    // resident reduced costs -> pricing from the potentials, once the re-hung subtrees have grown so large that patching
    // the reduced costs of their incident arcs costs more per pivot than the dearer sweeps (mcf_solve decides between batches)
    // candidate-list handles on the blocked list: pivots back to back in one workgroup while the updates are small (k_pivot_run)
    int run_pairs = 0;         // > 0: a list period is one sweep + this many (k_pivot_run, k_update_bpl) pairs; 0: one k_pivot per slot
    int run_low = 0;           // consecutive batches that made poor use of their run launches
    int run_pairs_cfg = 0;     // what mcf_create decided (a reset goes back to it)
    int64_t run_seen = 0;      // pivot count at the last look
    bool rc_able = false;      // the handle was created with resident reduced costs
    bool rc_dropped = false;   // ... and has stopped keeping them (until the next reset / warm start)
    int64_t rc_drop_subtree = 0;   // average |T2| over a batch from which on they are dropped (0: never)
    int64_t sw_pivots = 0, sw_subtree = 0;   // counters at the last look
    bool ctx_current = false;  // *h_ctx equals the device control block (no kernel was enqueued since it was read)
    bool external_driver = false;  // the caller enqueues the pivots itself (mcf_enqueue_*), possibly by replaying a graph it
                                   // captured: the library cannot know when the control block changes, so every read goes to the device
    // mcf_update_costs: everything allocated on first use
    std::vector<int32_t> uc_inv;     // caller's arc index -> engine arc index (inverse of im.orig)
    std::vector<uint32_t> uc_stamp;  // per engine arc: the call that last named it (duplicates: the last entry wins)
    uint32_t uc_gen = 0;
    int32_t *d_uc_arc = nullptr, *d_uc_cost = nullptr;   // the changes, engine indices
    int64_t uc_cap = 0;              // entries the two arrays hold
    McfJump* d_uc_jump[2] = {nullptr, nullptr};          // pointer-jumping records, double buffered
    int32_t* d_uc_info = nullptr;    // [0] greatest depth of the tree, [1] basic arcs among the changes
    // mcf_certify / mcf_bottlenecks: everything allocated on first use
    int64_t* d_ct_supply = nullptr;                        // [n]
    int64_t *d_ct_adj_off = nullptr, *d_ct_adj = nullptr;  // full adjacency, where the handle holds none or its shard's only
    int64_t *d_ct_flow = nullptr, *d_ct_pi = nullptr;      // the caller's arrays
    McfCertArcAcc* d_ct_arc = nullptr;                     // [kCertMaxBlocks + 1] per-workgroup partials, then the total
    McfCertNodeAcc* d_ct_node = nullptr;
    int32_t* d_ct_csum = nullptr;                          // [n_nodes]
    hipEvent_t ct_ev[3] = {nullptr, nullptr, nullptr};
    uint8_t* d_bn_flag = nullptr;                          // [m] bottleneck flag per caller's arc index
    int32_t* d_bn_cnt = nullptr;                           // per chunk of caller's indices
    int64_t* d_bn_off = nullptr;
    int64_t* d_bn_idx = nullptr;
    int64_t bn_idx_cap = 0;
    // mcf_certify_ray / mcf_certify_cut: everything allocated on first use (events, supplies and adjacency are the certificate's)
    McfRayAcc* d_ray_part = nullptr;                       // [kCertMaxBlocks + 1] per-workgroup partials, then the total
    int64_t* d_ray_idx = nullptr;                          // [n_nodes] the cycle in push order
    int32_t* d_cut_mark = nullptr;                         // [n] level at which the search reached the node, 0 = not in S
    int32_t* d_cut_level = nullptr;                        // [1] deepest level so far
    int8_t* d_cut_byte = nullptr;                          // [n] the caller's set going in, S_out coming back
    McfCutAcc* d_cut_part = nullptr;                       // [2 * kCertMaxBlocks + 1] arc partials, node partials, the total
    // mcf_update_rhs: everything allocated on first use (supplies and adjacency are the certificate's, jump records mcf_update_costs')
    std::vector<uint32_t> rhs_nstamp;                      // per node: the call that last named it
    int32_t* d_rhs_idx = nullptr;                          // changed nodes, then changed arcs (engine indices)
    int64_t* d_rhs_val = nullptr;                          // their new supplies / capacities
    int64_t rhs_cap = 0;                                   // entries the two arrays hold
    mcf_u128* d_rhs_bal = nullptr;                         // [n_nodes] balance per preorder position, then its prefix sums
    mcf_u128* d_rhs_part = nullptr;                        // per chunk of positions
    unsigned long long* d_rhs_info = nullptr;              // [RHS_COUNTERS]
    // mcf_update_rhs_dual: partials of the two choices, the phase's status record, the pivot log
    McfDualLeave* d_dual_leave = nullptr;                  // [kCertMaxBlocks + 1]
    McfDualEnter* d_dual_enter = nullptr;                  // [kMaxPriceBlocks]
    DualState* d_dual_state = nullptr;
    unsigned long long* d_dual_count = nullptr;            // arcs with a negative slack
    int64_t* d_dual_log = nullptr;                         // four words per pivot
    int64_t dual_log_cap = 0;                              // pivots the log holds
    // mcf_cost_ranges: everything allocated on first use (events are the certificate's)
    McfRngDepthAcc* d_rng_part = nullptr;                  // [kCertMaxBlocks + 1] per-workgroup partials, then the total
    unsigned long long* d_rng_info = nullptr;              // [RNG_COUNTERS]
    int32_t* d_rng_anc = nullptr;                          // [levels][n_nodes] binary-lifting ancestors
    int64_t *d_rng_p = nullptr, *d_rng_n = nullptr;        // [levels][n_nodes] the two min tables
    int64_t rng_cells = 0;                                 // levels * n_nodes the three tables hold
    int64_t *d_rng_down = nullptr, *d_rng_up = nullptr;    // [m] the answer in the caller's order
    int64_t rng_arcs = 0;                                  // entries the two arrays hold
    int64_t *d_rng_idx = nullptr, *d_rng_gdown = nullptr, *d_rng_gup = nullptr;   // an index list and its gathered answer
    int64_t rng_list = 0;                                  // entries the three arrays hold
    // mcf_supply_ranges / mcf_capacity_ranges: the ancestors and the two 8-byte tables above are shared (U = d_rng_p, D = d_rng_n)
    unsigned long long* d_frng_info = nullptr;             // [FRNG_COUNTERS]
    int32_t *d_frng_uid = nullptr, *d_frng_did = nullptr;  // [levels][n_nodes] the node whose tree arc attains the cell
    int64_t frng_cells = 0;                                // levels * n_nodes the two tables hold
    int64_t* d_frng_out = nullptr;                         // [5][m] down, up, down_arc, up_arc, rate in the caller's order
    int64_t frng_arcs = 0;                                 // m the array is laid out for
    int64_t *d_frng_idx = nullptr, *d_frng_gout = nullptr; // an index list [count] and its gathered answer [5][count]
    int64_t frng_list = 0;
    int32_t *d_frng_pair = nullptr, *d_frng_rise = nullptr;   // pairs: [2][count] from, to; [count] art_rising
    int64_t* d_frng_pout = nullptr;                        // [3][count] limit, limit_arc, rate
    int64_t frng_pairs = 0;
};

namespace {

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                        \
            return MCF_E_HIP;                                                                    \
        }                                                                                        \
    } while (0)

int usable_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

template <typename T>
hipError_t dalloc(T** p, size_t count) { return hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T)); }

// Measured on this stack (scripts/bin/hipcost): hipStreamCreate 3.7 ms, hipStreamDestroy 2.5 ms, hipHostFree 0.22 ms --
// against 4 ms for a whole netgen_8_08a solve and 16 us per instance in a batch (hipMalloc / hipFree: microseconds).
// Handles of small and mid-size instances therefore borrow a stream from a per-device pool (round robin, never
// destroyed) and their pinned control-block copy from a pool of slots; large handles keep a stream of their own.
constexpr int kPoolStreams = 4;
constexpr int kPooledMaxNodes = 1 << 14;
constexpr size_t kPinnedSlot = ((sizeof(McfCtx) + 63) & ~(size_t)63) + 64;   // control block + one candidate
std::mutex g_pool_mu;
std::vector<hipStream_t> g_pool_streams[64];    // per device
unsigned g_pool_next[64];
std::vector<char*> g_pinned_free;               // free slots

hipError_t pool_stream(int device, hipStream_t* out) {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    std::vector<hipStream_t>& v = g_pool_streams[device & 63];
    if ((int)v.size() < kPoolStreams) {
        hipStream_t s = nullptr;
        const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        v.push_back(s);
        *out = s;
        return hipSuccess;
    }
    *out = v[g_pool_next[device & 63]++ % kPoolStreams];
    return hipSuccess;
}

hipError_t pinned_take(char** out) {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (g_pinned_free.empty()) {
        constexpr int kSlots = 256;
        char* block = nullptr;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&block), kSlots * kPinnedSlot, hipHostMallocPortable);
        if (e != hipSuccess) return e;
        for (int i = kSlots - 1; i >= 0; --i) g_pinned_free.push_back(block + (size_t)i * kPinnedSlot);
    }
    *out = g_pinned_free.back();
    g_pinned_free.pop_back();
    return hipSuccess;
}
void pinned_give(char* slot) {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    g_pinned_free.push_back(slot);
}

// Host-to-device copies of an image go through a pinned staging buffer (one per host thread) when they fit: a copy from
// pageable memory costs ~34 us here whatever its size, from pinned memory a few (mcf_create of a small instance: ~15 copies).
constexpr size_t kStageBytes = (size_t)2 << 20;
struct Stage {
    char* base = nullptr;
    size_t used = 0;
    bool tried = false;
};
Stage g_stage;              // one per process (a per-thread one leaked 2 MiB of pinned memory for every host thread that ever created a handle)
std::mutex g_stage_mu;      // held by upload_image from its first staged copy to the synchronisation that ends it

hipError_t h2d(mcf_handle* h, void* dst, const void* src, size_t bytes) {
    Stage& st = g_stage;
    if (!st.tried) {
        st.tried = true;
        if (hipHostMalloc(reinterpret_cast<void**>(&st.base), kStageBytes, hipHostMallocPortable) != hipSuccess) { st.base = nullptr; (void)hipGetLastError(); }
    }
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (st.base && st.used + need <= kStageBytes) {
        char* p = st.base + st.used;
        st.used += need;
        std::memcpy(p, src, bytes);
        return hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, h->stream);
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream);
}

// the captured graph carries the view and the launch shapes by value: whatever changes either drops it, and the next
// batch captures a new one
void drop_graph(mcf_handle* h) {
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
    h->graph_batch = 0;
}

int upload_image(mcf_handle* h) {
    const McfHostImage& im = h->im;
    std::lock_guard<std::mutex> stage_lock(g_stage_mu);
    g_stage.used = 0;   // (everything staged below is synchronised before this function returns)
    if (h->rc_dropped) {   // a fresh start keeps the reduced costs resident again
        h->rc_dropped = false;
        h->rcached = true;
        h->overlap = h->overlap_cfg;
        h->view.rcache = h->d_rcache; h->view.vkey = h->d_vkey; h->view.dirty = h->d_dirty;
        drop_graph(h);
    }
    h->sw_pivots = 0; h->sw_subtree = 0;
    if (h->run_pairs != h->run_pairs_cfg) {   // (a fresh start gets the run shape back)
        h->run_pairs = h->run_pairs_cfg;
        drop_graph(h);
    }
    h->run_low = 0; h->run_seen = 0;
    HIP_TRY(h, h2d(h, h->d_tail, im.tail.data(), im.m_pad * 4));
    HIP_TRY(h, h2d(h, h->d_head, im.head.data(), im.m_pad * 4));
    HIP_TRY(h, h2d(h, h->d_cost, im.cost.data(), im.m_pad * 4));
    HIP_TRY(h, h2d(h, h->d_orig, im.orig.data(), im.m_pad * 4));
    HIP_TRY(h, h2d(h, h->d_state, im.state.data(), im.m_pad));
    HIP_TRY(h, h2d(h, h->d_weight, im.weight.data(), im.m_pad * 4));
    HIP_TRY(h, h2d(h, h->d_arcw, im.arcw.data(), im.arcw.size() * sizeof(McfArcW)));
    HIP_TRY(h, h2d(h, h->d_pi, im.pi.data(), im.pi.size() * 8));
    HIP_TRY(h, h2d(h, h->d_node, im.node.data(), im.node.size() * sizeof(McfNode)));
    std::vector<int32_t> reach;  // (outlives the asynchronous copy: synchronised at the end of this function)
    McfBplImage bp;              // (likewise)
    if (h->bpl) {
        // blocked preorder list: the dense image cut into blocks (slot = position), both meta copies alike, arena 1 empty
        mcf_bpl_build(im, h->bpl_shift, h->bpl_cap - h->bpl_dense > 0 ? h->bpl_cap - h->bpl_dense : -1, bp);
        if (bp.cap != h->bpl_cap || bp.shift != h->bpl_shift) { h->err = "internal: blocked-list geometry"; return MCF_E_INTERNAL; }
        HIP_TRY(h, hipMemcpyAsync(h->d_order0, bp.tok[0].data(), bp.tok[0].size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_psz0, bp.psz[0].data(), bp.psz[0].size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_psz1, 0, bp.psz[1].size() * 4, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_pos0, bp.loc.data(), bp.loc.size() * 4, hipMemcpyHostToDevice, h->stream));
        for (int a = 0; a < 2; ++a) {
            HIP_TRY(h, hipMemcpyAsync(h->d_bmeta[a], bp.meta[a].data(), bp.meta[a].size() * sizeof(McfBlkMeta), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(h->d_bext[a], bp.ext[a].data(), bp.ext[a].size() * 4, hipMemcpyHostToDevice, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // (pageable sources)
    } else {
    HIP_TRY(h, h2d(h, h->d_order0, im.order.data(), im.order.size() * 4));
    HIP_TRY(h, h2d(h, h->d_order1, im.order.data(), im.order.size() * 4));
    HIP_TRY(h, h2d(h, h->d_pos0, im.pos.data(), im.pos.size() * 4));
    HIP_TRY(h, h2d(h, h->d_pos1, im.pos.data(), im.pos.size() * 4));
    if (h->d_psz0) {
        HIP_TRY(h, h2d(h, h->d_psz0, im.psize.data(), im.psize.size() * 4));
        HIP_TRY(h, h2d(h, h->d_psz1, im.psize.data(), im.psize.size() * 4));
        if (h->d_reach) {
            const int64_t nb = ((int64_t)im.n_nodes + MCF_REACH_BLOCK - 1) / MCF_REACH_BLOCK;
            reach.assign((size_t)nb, 0);
            for (int64_t j = 0; j < im.n_nodes; ++j) {
                const int32_t end = (int32_t)(j + im.psize[j]);
                if (end > reach[j >> MCF_REACH_SHIFT]) reach[j >> MCF_REACH_SHIFT] = end;
            }
            HIP_TRY(h, h2d(h, h->d_reach, reach.data(), reach.size() * 4));
        }
    }
    }
    if (h->rcached)
        HIP_TRY(h, h2d(h, h->d_rcache, im.rcache.data(), im.m_pad * 8));
    std::vector<int32_t> vk;  // (synchronised before this function returns)
    if (h->d_vkey) {
        vk.assign(im.m_pad, 0);
        for (int64_t e = 0; e < im.m; ++e) vk[e] = mcf_vkey(-(int64_t)im.state[e] * im.rcache[e], h->view.vk_bigm, h->view.vk_half);
        HIP_TRY(h, h2d(h, h->d_vkey, vk.data(), vk.size() * 4));
    }
    if (h->d_dirty) HIP_TRY(h, hipMemsetAsync(h->d_dirty->flag, 1, sizeof(h->d_dirty->flag), h->stream));  // every block is due (any non-zero word)
    if (h->d_swept) HIP_TRY(h, hipMemsetAsync(h->d_swept, 0, kMaxPriceBlocks * sizeof(int64_t), h->stream));
    McfCtx c;
    std::memset(&c, 0, sizeof c);
    c.unbounded_arc = -1;
    const int64_t m = im.m;
    mcf_init_block_state(&c, h->opt.rule, m, h->opt.block_size);
    if (h->opt.rule == MCF_RULE_DEVEX_BLOCK) {
        if (h->opt.devex_tuner > 0) c.auto_tune = 1; else if (h->opt.devex_tuner < 0) c.auto_tune = 0;
        if (h->opt.devex_stay > 0) c.devex_cyclic = 0;
    }
    // (the fused LDS loop has no pricing grid: its candidate list is one entry per head bucket whatever price_blocks asks for,
    //  and the minor pivots per sweep follow the length of the list that is really kept)
    c.minor_cap = mcf_minor_cap(h->small ? MCF_NUM_BUCKETS : h->price_blocks);
    c.climb_budget = h->climb_budget;
    // shallow end points are climbed outright: one round trip per level beats the scan's fixed passes up to ~3 levels at
    // mid size (one plain round) and ~8 levels where the coarse index is used (two passes over up to 16 K words first)
    c.climb_depth = h->opt.climb_depth > 0 ? h->opt.climb_depth : (h->opt.climb_depth < 0 ? 0 : (im.n_nodes > 32768 ? 8 : 3));
    if (h->bpl) { c.arena = 0; c.alloc_next = h->bpl_dense; c.dense_blocks = h->bpl_dense; }
    *h->h_ctx = c;
    if (h->shards > 1 && !h->d_full_tab) {
        int32_t tab[MCF_NUM_BUCKETS * 2];
        for (int x = 0; x < MCF_NUM_BUCKETS; ++x) {
            int64_t lo, hi;
            mcf_bucket_slice(im.bucket_off, x, h->shard, h->shards, 0, 1, &lo, &hi);
            tab[x * 2] = (int32_t)lo; tab[x * 2 + 1] = (int32_t)hi;
        }
        if (dalloc(&h->d_full_tab, MCF_NUM_BUCKETS * 2) != hipSuccess) { h->err = "hipMalloc slice table"; return MCF_E_ALLOC; }
        HIP_TRY(h, hipMemcpy(h->d_full_tab, tab, sizeof tab, hipMemcpyHostToDevice));
    }
    if (h->d_dx && !h->dx_filled) {  // granule table, once
        McfDevex* dx = new (std::nothrow) McfDevex();
        if (!dx) { h->err = "host allocation"; return MCF_E_ALLOC; }
        std::memset(dx, 0, sizeof *dx);
        mcf_devex_fill_granules(dx, im.bucket_off);
        const hipError_t de = hipMemcpy(h->d_dx, dx, sizeof *dx, hipMemcpyHostToDevice);
        delete dx;
        if (de != hipSuccess) { h->err = "copy granule table"; return MCF_E_HIP; }
        h->dx_filled = true;
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_ctx, h->h_ctx, sizeof(McfCtx), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // per-pass accounting: a Devex pass prices one block of the shard, Dantzig the whole shard
    h->shard_arcs = 0;
    for (int x = 0; x < MCF_NUM_BUCKETS; ++x) {
        int64_t lo, hi;
        mcf_bucket_slice(im.bucket_off, x, h->shard, h->shards, 0, 1, &lo, &hi);
        h->shard_arcs += hi - lo;
    }
    h->priced_per_pass = h->opt.rule == MCF_RULE_DEVEX_BLOCK ? h->shard_arcs * c.block_granules / MCF_GRANULES : h->shard_arcs;
    std::memset(&h->stats, 0, sizeof h->stats);
    h->stats.unbounded_arc = -1;
    {   // compulsory bytes of ONE pricing launch of this handle's sweep kernel
        const bool devex = h->opt.rule == MCF_RULE_DEVEX_BLOCK;
        if (h->d_vkey && !devex) h->stats.price_bytes = 4 * h->priced_per_pass;                       // k_price_v: key codes
        else if (h->rcached) h->stats.price_bytes = (devex ? 13 : 9) * h->priced_per_pass;            // k_price_rc: rc + state (+ weight)
        else h->stats.price_bytes = (devex ? 17 : 13) * h->priced_per_pass + 8 * (int64_t)im.n_nodes; // k_price: SURVEY 8d's gather figure
    }
    h->total_cap = 0;
    h->solved_once = false;
    h->ctx_current = true;  // *h_ctx was just copied to the device
    h->external_driver = false;
    return MCF_OK;
}

void launch_price(mcf_handle* h, hipStream_t s, const McfView& v_in, int32_t rule, int use_block, McfCand* out = nullptr) {
    int64_t* swept = out ? nullptr : h->d_swept;  // measurement / parity launches (own candidate buffer) are not accounted
    McfView vx = v_in;
    if (out) vx.candx = nullptr;   // ... and leave the live list's records alone
    const McfView& v = vx;
    if (!out) out = h->d_cand;
    const dim3 grid(h->price_blocks), block(kPriceThreads);
    const int64_t z = 0;
    // use_block: 0 = whole shard, 1 = current Devex block, 2 = whole shard unless minor iterations are pending
    if (rule == MCF_RULE_CANDIDATE_LIST && use_block) use_block = 2;
    if (h->rcached && v.vkey && rule != MCF_RULE_DEVEX_BLOCK) {
        const bool nt = h->nt_sweep;
        if (v.dirty) hipLaunchKernelGGL((k_price_v<true>), grid, block, 0, s, v, h->shard, h->shards, use_block, out, swept, (const int32_t*)h->d_full_tab);
        else if (nt) hipLaunchKernelGGL((k_price_v<false, true>), grid, block, 0, s, v, h->shard, h->shards, use_block, out, swept, (const int32_t*)h->d_full_tab);
        else hipLaunchKernelGGL((k_price_v<false>), grid, block, 0, s, v, h->shard, h->shards, use_block, out, swept, (const int32_t*)h->d_full_tab);
    } else if (h->rcached) {
        if (rule == MCF_RULE_DEVEX_BLOCK)
            hipLaunchKernelGGL((k_price_rc<MCF_RULE_DEVEX_BLOCK, false, false>), grid, block, 0, s, v, h->shard, h->shards, use_block, z, z, out, swept, (const int32_t*)nullptr);
        else
            if (v.dirty) hipLaunchKernelGGL((k_price_rc<MCF_RULE_DANTZIG, false, true>), grid, block, 0, s, v, h->shard, h->shards, use_block, z, z, out, swept, (const int32_t*)h->d_full_tab);
            else hipLaunchKernelGGL((k_price_rc<MCF_RULE_DANTZIG, false, false>), grid, block, 0, s, v, h->shard, h->shards, use_block, z, z, out, swept, (const int32_t*)h->d_full_tab);
    } else {
        if (rule == MCF_RULE_DEVEX_BLOCK)
            hipLaunchKernelGGL((k_price<MCF_RULE_DEVEX_BLOCK, false>), grid, block, 0, s, v, h->shard, h->shards, use_block, z, z, out);
        else
            hipLaunchKernelGGL((k_price<MCF_RULE_DANTZIG, false>), grid, block, 0, s, v, h->shard, h->shards, use_block, z, z, out);
    }
}

void launch_k_pivot(mcf_handle* h, hipStream_t s, const McfCand* cand, int ncand, int32_t rule, int have_sweep) {
    const McfCand* own = h->d_cand;
    const dim3 one(1), block(kPivotThreads);
    if (h->view.dirty) {
        if (h->bpl) hipLaunchKernelGGL((k_pivot<true, true>), one, block, 0, s, h->view, cand, ncand, rule, have_sweep, own);
        else hipLaunchKernelGGL((k_pivot<true, false>), one, block, 0, s, h->view, cand, ncand, rule, have_sweep, own);
    } else {
        if (h->bpl) hipLaunchKernelGGL((k_pivot<false, true>), one, block, 0, s, h->view, cand, ncand, rule, have_sweep, own);
        else hipLaunchKernelGGL((k_pivot<false, false>), one, block, 0, s, h->view, cand, ncand, rule, have_sweep, own);
    }
}

void launch_apply(mcf_handle* h, hipStream_t s) {
    if (h->bpl) {  // blocked preorder list: block records, T2 move and reduced-cost patch in one launch
        const dim3 grid(h->bpl_grid + 1 + (h->view.candx ? 1 : 0)), block(kBplThreads);   // (+1: the direct workgroup, +1: the candidate cache)
        if (!h->rcached) hipLaunchKernelGGL((k_update_bpl<false, false>), grid, block, 0, s, h->view, h->bpl_grid);
        else if (h->view.dirty) hipLaunchKernelGGL((k_update_bpl<true, true>), grid, block, 0, s, h->view, h->bpl_grid);
        else hipLaunchKernelGGL((k_update_bpl<false, true>), grid, block, 0, s, h->view, h->bpl_grid);
        return;
    }
    const int xb = h->view.candx ? kCandxBlocks : 0;
    if (h->rcached) {  // tree/potential update and reduced-cost update in one launch
        if (h->view.dirty) hipLaunchKernelGGL(k_update<true>, dim3(h->apply_blocks + h->rcupd_blocks + xb), dim3(kRcupdThreads), 0, s, h->view, h->apply_blocks);
        else hipLaunchKernelGGL(k_update<false>, dim3(h->apply_blocks + h->rcupd_blocks + xb), dim3(kRcupdThreads), 0, s, h->view, h->apply_blocks);
    } else {
        hipLaunchKernelGGL(k_apply, dim3(h->apply_blocks + xb), dim3(kApplyThreads), 0, s, h->view);
    }
}

// One list period in "run" shape: the sweep (a no-op while the list is live), then `run_pairs` pairs of (pivots back to back
// until an update is too large for one workgroup or the list is used up, that update on the grid).
void launch_run_period(mcf_handle* h, hipStream_t s) {
    const int32_t rule = h->opt.rule;
    const int steps = mcf_minor_cap(h->price_blocks) + 1;
    launch_price(h, s, h->view, rule, 1);
    for (int i = 0; i < h->run_pairs; ++i) {
        const dim3 one(1), block(kPivotThreads);
        const int sweep = i == 0 ? 1 : 0;
        if (h->rcached) {
            if (h->view.dirty) hipLaunchKernelGGL((k_pivot_run<true, true>), one, block, 0, s, h->view, h->price_blocks, sweep, steps);
            else hipLaunchKernelGGL((k_pivot_run<false, true>), one, block, 0, s, h->view, h->price_blocks, sweep, steps);
        } else {
            hipLaunchKernelGGL((k_pivot_run<false, false>), one, block, 0, s, h->view, h->price_blocks, sweep, steps);
        }
        launch_apply(h, s);
    }
}

// One pivot slot.  Candidate-list rule: only every (minor_cap + 1)-th slot carries a pricing launch;
// the slots in between go straight to k_pivot, which re-prices the list (a pricing launch there
// would be a no-op anyway -- this just saves its launch boundary).
// arm_cap >= 0 (persistent loop outside a graph): the kernel takes the pivot cap from its argument, no k_ctl launch
void launch_pivot_triplet(mcf_handle* h, hipStream_t s, int slot = 0, int64_t arm_cap = -1) {
    const int32_t rule = h->opt.rule;
    if (h->mid) {
        // candidate list: one grid sweep (a no-op while the list is live), then the persistent loop runs the major
        // pivot and every minor pivot the list yields.  Other rules: the loop prices by itself until the solve ends.
        const bool listing = rule == MCF_RULE_CANDIDATE_LIST;
        if (listing) launch_price(h, s, h->view, rule, 1);
        hipLaunchKernelGGL(k_solve_mid, dim3(1), dim3(kPivotThreads), 0, s, h->view, rule, h->d_cand, h->price_blocks,
                           listing ? 1 : 0, listing ? mcf_minor_cap(h->price_blocks) + 2 : (1 << 22), arm_cap >= 0 ? 1 : 0,
                           arm_cap >= 0 ? arm_cap : (int64_t)0);
        return;
    }
    int have_sweep = 1;
    if (rule == MCF_RULE_CANDIDATE_LIST) have_sweep = slot % (mcf_minor_cap(h->price_blocks) + 1) == 0;
    if (have_sweep) launch_price(h, s, h->view, rule, rule != MCF_RULE_DANTZIG);
    launch_k_pivot(h, s, h->d_cand, h->price_blocks, rule, have_sweep);
    launch_apply(h, s);
}

int build_graph(mcf_handle* h, int batch) {
    if (h->graph_exec && h->graph_batch == batch) return MCF_OK;
    drop_graph(h);
    if (h->overlap) {
        while (h->fork_ev.size() < (size_t)batch * 2) {
            hipEvent_t e;
            HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->fork_ev.push_back(e);
        }
    }
    HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    if (h->run_pairs > 0) {
        const int period = mcf_minor_cap(h->price_blocks) + 1;
        for (int i = 0; i < batch / period; ++i) launch_run_period(h, h->stream);
    } else if (!h->overlap) {
        for (int i = 0; i < batch; ++i) launch_pivot_triplet(h, h->stream, i);
    } else {
        // main:  [price 0] pivot t -> permutation t ------------------------> pivot t+1 ...
        // side:            \-> reduced-cost patch t -> price t+1 ---------/
        // k_price reads what k_pivot and the patch wrote (control block, states, weights, reduced costs / key codes, dirty
        // flags); the permutation writes order / pos / psz / pi / reach only, which pricing from resident values never reads.
        const int32_t rule = h->opt.rule;
        launch_price(h, h->stream, h->view, rule, rule != MCF_RULE_DANTZIG);
        for (int i = 0; i < batch; ++i) {
            hipEvent_t pivoted = h->fork_ev[(size_t)i * 2], priced = h->fork_ev[(size_t)i * 2 + 1];
            launch_k_pivot(h, h->stream, h->d_cand, h->price_blocks, rule, 1);
            HIP_TRY(h, hipEventRecord(pivoted, h->stream));
            HIP_TRY(h, hipStreamWaitEvent(h->side, pivoted, 0));
            if (h->view.dirty) hipLaunchKernelGGL(k_rcupd<true>, dim3(h->rcupd_blocks), dim3(kRcupdThreads), 0, h->side, h->view);
            else hipLaunchKernelGGL(k_rcupd<false>, dim3(h->rcupd_blocks), dim3(kRcupdThreads), 0, h->side, h->view);
            if (i + 1 < batch) launch_price(h, h->side, h->view, rule, rule != MCF_RULE_DANTZIG);
            HIP_TRY(h, hipEventRecord(priced, h->side));
            hipLaunchKernelGGL(k_apply, dim3(h->apply_blocks), dim3(kApplyThreads), 0, h->stream, h->view);
            HIP_TRY(h, hipStreamWaitEvent(h->stream, priced, 0));
        }
    }
    HIP_TRY(h, hipStreamEndCapture(h->stream, &h->graph));
    HIP_TRY(h, hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    h->graph_batch = batch;
    return MCF_OK;
}

// One batch of pivots with every kernel bracketed by events (profile mode).
int run_batch_profiled(mcf_handle* h, int batch) {
    const size_t need = (size_t)batch * 4;
    while (h->events.size() < need) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreate(&e));
        h->events.push_back(e);
    }
    const int32_t rule = h->opt.rule;
    for (int i = 0; i < batch; ++i) {
        hipEvent_t* ev = &h->events[(size_t)i * 4];
        HIP_TRY(h, hipEventRecord(ev[0], h->stream));
        launch_price(h, h->stream, h->view, rule, rule != MCF_RULE_DANTZIG);
        HIP_TRY(h, hipEventRecord(ev[1], h->stream));
        launch_k_pivot(h, h->stream, h->d_cand, h->price_blocks, rule, 1);
        HIP_TRY(h, hipEventRecord(ev[2], h->stream));
        launch_apply(h, h->stream);
        HIP_TRY(h, hipEventRecord(ev[3], h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < batch; ++i) {
        hipEvent_t* ev = &h->events[(size_t)i * 4];
        float a = 0, b = 0, c = 0;
        (void)hipEventElapsedTime(&a, ev[0], ev[1]);
        (void)hipEventElapsedTime(&b, ev[1], ev[2]);
        (void)hipEventElapsedTime(&c, ev[2], ev[3]);
        h->stats.price_ms += a; h->stats.pivot_ms += b; h->stats.apply_ms += c;
    }
    h->stats.price_launches += batch; h->stats.pivot_launches += batch; h->stats.apply_launches += batch;
    return MCF_OK;
}

int read_ctx(mcf_handle* h, hipStream_t s) {
    HIP_TRY(h, hipMemcpyAsync(h->h_ctx, h->d_ctx, sizeof(McfCtx), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->ctx_current = true;
    return MCF_OK;
}
// the host copy of the control block, refreshed only when something ran since it was last read
int sync_ctx(mcf_handle* h, hipStream_t s) { return (h->ctx_current && !h->external_driver) ? MCF_OK : read_ctx(h, s); }

// Which copies of the preorder arrays hold the tree mcf_get_tree reports, a flip the last update left pending counted (c must be
// current).  cur: dense position / order / size arrays and the blocked list's block table; arena: its slot arena.
struct TreeSel { int32_t cur, arena; };
TreeSel tree_sel(const McfCtx& c) {
    return {c.cur ^ (c.pending_flip ? 1 : 0), c.arena ^ ((c.pending_flip && c.rebuild) ? 1 : 0)};
}

void free_all(mcf_handle* h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);   // (a borrowed stream may still hold this handle's work)
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->fork_ev) (void)hipEventDestroy(e);
    if (h->side) (void)hipStreamDestroy(h->side);
    for (hipEvent_t e : h->loop_ev) if (e) (void)hipEventDestroy(e);
    (void)hipFree(h->d_tail); (void)hipFree(h->d_head); (void)hipFree(h->d_cost); (void)hipFree(h->d_orig); (void)hipFree(h->d_state); (void)hipFree(h->d_prio); (void)hipFree(h->d_weight);
    (void)hipFree(h->d_arcw); (void)hipFree(h->d_pi); (void)hipFree(h->d_node); (void)hipFree(h->d_order0); (void)hipFree(h->d_order1);
    (void)hipFree(h->d_path1); (void)hipFree(h->d_path2); (void)hipFree(h->d_ppos1); (void)hipFree(h->d_ppos2); (void)hipFree(h->d_rec1); (void)hipFree(h->d_rec2); (void)hipFree(h->d_seg); (void)hipFree(h->d_ctx); (void)hipFree(h->d_cand); (void)hipFree(h->d_cand_aux); (void)hipFree(h->d_one);
    (void)hipFree(h->d_pos0); (void)hipFree(h->d_pos1); (void)hipFree(h->d_psz0); (void)hipFree(h->d_psz1); (void)hipFree(h->d_reach); (void)hipFree(h->d_chg); (void)hipFree(h->d_dirty); (void)hipFree(h->d_swept); (void)hipFree(h->d_dx); (void)hipFree(h->d_full_tab);
    (void)hipFree(h->d_rcache); (void)hipFree(h->d_adj_off); (void)hipFree(h->d_adj); (void)hipFree(h->d_vkey); (void)hipFree(h->d_candx);
    for (int a = 0; a < 2; ++a) { (void)hipFree(h->d_bmeta[a]); (void)hipFree(h->d_bext[a]); }
    (void)hipFree(h->d_ct_supply); (void)hipFree(h->d_ct_adj_off); (void)hipFree(h->d_ct_adj); (void)hipFree(h->d_ct_flow); (void)hipFree(h->d_ct_pi);
    (void)hipFree(h->d_ct_arc); (void)hipFree(h->d_ct_node); (void)hipFree(h->d_ct_csum);
    (void)hipFree(h->d_bn_flag); (void)hipFree(h->d_bn_cnt); (void)hipFree(h->d_bn_off); (void)hipFree(h->d_bn_idx);
    for (hipEvent_t e : h->ct_ev) if (e) (void)hipEventDestroy(e);
    (void)hipFree(h->d_uc_arc); (void)hipFree(h->d_uc_cost); (void)hipFree(h->d_uc_jump[0]); (void)hipFree(h->d_uc_jump[1]); (void)hipFree(h->d_uc_info);
    (void)hipFree(h->d_ray_part); (void)hipFree(h->d_ray_idx); (void)hipFree(h->d_cut_mark); (void)hipFree(h->d_cut_level); (void)hipFree(h->d_cut_byte); (void)hipFree(h->d_cut_part);
    (void)hipFree(h->d_rhs_idx); (void)hipFree(h->d_rhs_val); (void)hipFree(h->d_rhs_bal); (void)hipFree(h->d_rhs_part); (void)hipFree(h->d_rhs_info);
    (void)hipFree(h->d_dual_leave); (void)hipFree(h->d_dual_enter); (void)hipFree(h->d_dual_state); (void)hipFree(h->d_dual_count); (void)hipFree(h->d_dual_log);
    (void)hipFree(h->d_rng_part); (void)hipFree(h->d_rng_info); (void)hipFree(h->d_rng_anc); (void)hipFree(h->d_rng_p); (void)hipFree(h->d_rng_n);
    (void)hipFree(h->d_rng_down); (void)hipFree(h->d_rng_up); (void)hipFree(h->d_rng_idx); (void)hipFree(h->d_rng_gdown); (void)hipFree(h->d_rng_gup);
    (void)hipFree(h->d_frng_info); (void)hipFree(h->d_frng_uid); (void)hipFree(h->d_frng_did); (void)hipFree(h->d_frng_out); (void)hipFree(h->d_frng_idx);
    (void)hipFree(h->d_frng_gout); (void)hipFree(h->d_frng_pair); (void)hipFree(h->d_frng_rise); (void)hipFree(h->d_frng_pout);
    if (h->h_ctx) pinned_give(reinterpret_cast<char*>(h->h_ctx));   // (h_one lives in the same slot)
    if (h->stream && h->stream_owned) (void)hipStreamDestroy(h->stream);
}

// LDS plan of the fused small-instance path: mcf_small_plan (mcf_core.h), which also checks what the 256-lane front kernel's
// pair arithmetic and packed counts rest on
bool small_plan(int64_t m_pad, size_t arcw_count, int32_t n_nodes, bool devex, SmallLayout* out) {
    return mcf_small_plan(m_pad, (uint64_t)arcw_count, n_nodes, devex, out);
}

// Width of the fused loop's workgroup, from the measured table in DESIGN.md (k_solve_small).  One wave per SIMD (256 lanes)
// reduces over 4 waves instead of 16 and meets 4 arrivals at each barrier; four waves per SIMD (1 024 lanes) hide the LDS round
// trips of a sweep that reads its arcs from LDS (Devex) and of the passes over a larger tree -- but since every wave takes the
// scalar decisions of a pivot itself, sixteen waves repeat them on four SIMDs and keep the control block in scalar registers
// that spill (small_scalar_control): 256 lanes won at 65, 257 and 514 tree nodes under every rule, by 0.5 to 1.8 us per pivot.
// MCF_SMALL_THREADS = 256 / 1024 forces a width, for mcf_solve (read at mcf_create) and for mcf_solve_batch (read at the call).
int small_threads_forced() {   // 0: no valid MCF_SMALL_THREADS
    if (const char* st = std::getenv("MCF_SMALL_THREADS")) {
        const int w = std::atoi(st);
        if (w == 256 || w == 1024) return w;
    }
    return 0;
}
int small_threads_for(int32_t n_nodes, int32_t rule) {
    if (const int w = small_threads_forced()) return w;
    (void)n_nodes; (void)rule;   // (no measured size or rule at which 1 024 lanes win any more)
    return 256;
}

// 32-bit pricing keys in the fused loop (the narrow sweep of solve_small_body): MCF_SMALL_NARROW=0 forces the 64-bit path -- read
// where MCF_SMALL_THREADS is read, at mcf_create for mcf_solve and at the call for mcf_solve_batch -- otherwise the instance
// decides, at every launch: big-M grows on a resident handle (mcf_update_costs, mcf_add_arcs).  max|cost| is taken from the
// invariant big-M >= (max|cost| + 1)(n + 2), which is exact on a fresh handle and an upper bound after costs came down.
bool small_narrow_allowed() {
    const char* sn = std::getenv("MCF_SMALL_NARROW");
    return !(sn && sn[0] == '0' && sn[1] == '\0');
}
// the bit fields of small_info (device): 11 bits per node, 9 per slot of a lane at the narrowest bucket share (32 lanes)
bool small_info_fits(int32_t n_nodes, int64_t m_pad) { return n_nodes <= 2048 && m_pad / 32 < 512; }
int32_t small_narrow_for(const McfHostImage& im, bool allowed) {
    const int64_t max_abs = im.big_m / ((int64_t)im.n + 2) - 1;
    return allowed && small_info_fits(im.n_nodes, im.m_pad) && mcf_small_narrow_fits(im.big_m, max_abs) ? 1 : 0;
}

// Which kernel: the front kernel (k_solve_small<.., true>) for Dantzig with the plain key on a range that fits.  The front kernel
// sets the view's Devex pointers to null at compile time: a view that carries weights never takes it (mcf_create gives weights
// to MCF_RULE_DEVEX_BLOCK only, so this refuses nothing today -- it states what the kernel relies on).
bool small_front_for(int32_t narrow, int32_t rule, int32_t key_mode, const McfView& view) {
    return narrow != 0 && rule == MCF_RULE_DANTZIG && key_mode == MCF_KEY_PLAIN && !view.weight && !view.dx;
}
// The instantiation for a width (256 unless 1 024 is forced) and a front, one instance per launch / one per workgroup.
auto small_kernel(int threads, bool front) {
    if (threads == 1024) return front ? k_solve_small<1024, true> : k_solve_small<1024, false>;
    return front ? k_solve_small<256, true> : k_solve_small<256, false>;
}
auto small_batch_kernel(int threads, bool front) {
    if (threads == 1024) return front ? k_solve_small_batch<1024, true> : k_solve_small_batch<1024, false>;
    return front ? k_solve_small_batch<256, true> : k_solve_small_batch<256, false>;
}

// The dynamic-LDS limit of the fused kernels covers `total` bytes on this device.  (The limit is a property of the kernel,
// not of the handle: it only ever grows, so that handles of different sizes can be alive together -- and share one batched launch.)
bool small_reserve(int device, uint32_t total) {
    static std::mutex lds_mu;
    static int lds_limits[64] = {0};   // per device: the attribute belongs to the device's copy of the function
    int& lds_limit = lds_limits[device & 63];
    std::lock_guard<std::mutex> lock(lds_mu);
    if ((int)total <= lds_limit) return true;
    hipError_t fe = hipSuccess;
    for (int threads : {256, 1024})
        for (bool front : {false, true})
            for (const void* fn : {reinterpret_cast<const void*>(small_kernel(threads, front)), reinterpret_cast<const void*>(small_batch_kernel(threads, front))})
                if (fe == hipSuccess) fe = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)total);
    if (fe != hipSuccess) { (void)hipGetLastError(); return false; }   // (the refusal must not surface later as some launch's error)
    lds_limit = (int)total;
    return true;
}

// ====================================================================== mcf_create in three parts
// decide_geometry: everything that decides which arrays exist, how long they are and which kernels run, from the image and
// the options (and the environment's A/B switches);  alloc_wire: the one place that allocates the solver's device arrays
// and wires McfView;  upload_image (above): the start state.  mcf_fork runs alloc_wire on a copy of the source's image,
// options and geometry (inherit_geometry: nothing is read from the environment again) and a device copy in place of the upload.
std::vector<std::pair<const char*, int64_t>> shape_of(const mcf_handle* h) {
    return {{"n", h->im.n}, {"m", h->im.m}, {"padded m", h->im.m_pad}, {"device", h->device}, {"rule", h->opt.rule}, {"key_mode", h->key_mode},
            {"engine path (fused LDS loop)", h->small}, {"fused loop width", h->small_threads}, {"engine path (persistent mid loop)", h->mid},
            {"tree layout", h->bpl}, {"tree block shift", h->bpl_shift}, {"tree blocks", h->bpl_cap}, {"dense tree blocks", h->bpl_dense},
            {"tree update grid", h->bpl_grid}, {"cycle scan", h->scan_ok}, {"resident reduced costs", h->rc_able}, {"key codes", h->want_vkey},
            {"dirty marks", h->want_dirty}, {"candidate cache", h->want_candx}, {"arc priorities", h->d_prio != nullptr},
            {"pricing grid", h->price_blocks}, {"apply grid", h->apply_blocks}, {"reduced-cost update grid", h->rcupd_blocks},
            {"overlapped graphs", h->overlap_cfg}, {"shard_count", h->shards}, {"own stream", h->stream_owned}};
}

void decide_geometry(mcf_handle* h) {
    const McfHostImage& im = h->im;
    const mcf_options& opt = h->opt;
    const int64_t m = im.m;
    {
        // Tree layout: the blocked preorder list (mcf_core.h) from kBplMinNodes nodes on -- below that the dense array's block
        // permutation moves few enough positions, and the persistent loops keep the dense array anyway.
        // tree_blocks: 0 = auto, -1 = dense array, k >= 2 = blocks of 2^k slots;  tree_pool: spare blocks (0 = auto, -1 = none).
        const bool forced = opt.tree_blocks > 0, never = opt.tree_blocks < 0;
        h->bpl = !never && opt.mid_loop <= 0 && opt.overlap_update <= 0 && (forced || im.n_nodes >= kBplMinNodes);
        if (h->bpl) {
            int32_t sh = 0, cap = 0, dense = 0;
            mcf_bpl_geometry(im.n_nodes, forced ? opt.tree_blocks : 0, opt.tree_pool, &sh, &cap, &dense);
            h->bpl_shift = sh; h->bpl_cap = cap; h->bpl_dense = dense;
            // (a large grid costs dispatch time on every pivot: 1 M / 16 M, 256 -> 64 workgroups: k_update_bpl 7.5 -> 6.0 us, +4 % pivots/s)
            int g = (cap + 7) / 8;
            if (g > 64) g = 64;
            if (const char* ge = std::getenv("MCF_BPL_GRID")) { const int vv = std::atoi(ge); if (vv >= 1 && vv <= 4096) g = vv; }   // A/B switch
            if (g < 1) g = 1;
            while ((cap + g - 1) / g > kBplTouchedCap) g *= 2;
            h->bpl_grid = g;
        }
    }
    {
        // 8 * k workgroups, one group of k per XCD head bucket (formula shared with the CPU emulation)
        h->price_blocks = mcf_price_blocks(m, h->shards, opt.price_blocks);
        const int64_t ab = ((int64_t)im.n_nodes + kApplyThreads - 1) / kApplyThreads;
        int max_ab = kMaxApplyBlocks;
        if (const char* ab_env = std::getenv("MCF_APPLY_BLOCKS")) { const int vv = std::atoi(ab_env); if (vv >= 64 && vv <= 4096) max_ab = vv; }   // A/B switch
        h->apply_blocks = (int)(ab < max_ab ? ab : max_ab);
    }
    h->stream_owned = im.n > kPooledMaxNodes;
    h->key_mode = opt.key_mode > 0 ? opt.key_mode : (opt.forward_first ? MCF_KEY_FORWARD_FIRST : MCF_KEY_PLAIN);
    // the fused small-instance path: its LDS plan, and the kernels' dynamic-LDS limit raised to it (refused: the three-kernel GPU path)
    h->small = !h->bpl && !opt.no_fused && !opt.profile && h->shards == 1 &&
               small_plan(im.m_pad, im.arcw.size(), im.n_nodes, opt.rule == MCF_RULE_DEVEX_BLOCK, &h->small_layout) &&
               small_reserve(h->device, h->small_layout.total);
    if (h->small) { h->small_threads = small_threads_for(im.n_nodes, opt.rule); h->small_narrow_ok = small_narrow_allowed(); }
    // position-space subtree sizes for the cycle scan: every handle but the LDS-resident ones
    h->scan_ok = opt.cycle_scan >= 0 && im.n_nodes <= kScanMaxNodes && !h->small;  // -1: never scan
    // cycle search: how many round trips the one-lane climb takes before the workgroup-wide scan over
    // preorder positions finishes the cycle.  Auto = none: measured on MI355X (profiles/r01_f_*), scanning
    // at once beats every hybrid from 256 to 65 536 nodes -- a dependent global round trip per tree level
    // costs more than the whole scan's ~4 -- by 1.1x (netgen_8_08a) to 4.5x (goto_8_16a, cycles of ~450 arcs).
    if (!h->scan_ok && !(h->bpl && opt.cycle_scan >= 0)) h->climb_budget = INT32_MAX;
    else if (opt.cycle_scan > 0) h->climb_budget = opt.cycle_scan - 1;
    else h->climb_budget = 0;
    // resident reduced costs for everything that does not take the fused LDS path
    h->rcached = !h->small && !opt.no_rcache && im.m > 0;
    h->rc_able = h->rcached;
    // a rank patches only the reduced costs it sweeps -- for the rules whose sweeps cover a FIXED share of every bucket.
    // Devex cuts the block first and the shard second (so that the union over ranks does not depend on the rank
    // count), and blocks move and resize: there every rank keeps all reduced costs exact, as a single GPU does.
    h->rc_partial = h->rcached && h->shards > 1 && opt.rule != MCF_RULE_DEVEX_BLOCK;
    if (h->rcached) {
        const int64_t rb = ((int64_t)im.n_nodes + 15) / 16;  // one 16-lane group per node of the largest possible T2
        int max_rb = kMaxRcupdBlocks;
        if (const char* re = std::getenv("MCF_RCUPD_BLOCKS")) { const int vv = std::atoi(re); if (vv >= 1 && vv <= 4096) max_rb = vv; }   // A/B switch
        h->rcupd_blocks = (int)(rb < max_rb ? (rb > 0 ? rb : 1) : max_rb);
    }
    // persistent single-workgroup loop: the tree work of one pivot must be small enough for one CU, and so must
    // the arcs it prices per pivot (a Devex block / the whole arc list for Dantzig; the candidate list's full
    // sweeps stay on the grid)
    {
        int64_t per_pivot_arcs = 0;
        if (opt.rule == MCF_RULE_DEVEX_BLOCK) {
            McfCtx probe;  // the largest block the tuner may grow to (mcf_core.h: never beyond MCF_TUNER_MAX_ARCS or the initial size)
            std::memset(&probe, 0, sizeof probe);
            mcf_init_block_state(&probe, opt.rule, im.m, opt.block_size);
            per_pivot_arcs = im.m * probe.max_granules / MCF_GRANULES;
        } else if (opt.rule == MCF_RULE_DANTZIG_FULL) {
            per_pivot_arcs = im.m;
        }
        // (the candidate list never gains from the loop -- its full sweeps run on the grid either way -- and stays on the graph)
        const bool fits = im.n_nodes <= kMidMaxNodes && per_pivot_arcs <= kMidMaxArcsPerPivot && opt.rule != MCF_RULE_CANDIDATE_LIST;
        h->mid = !h->bpl && h->rcached && h->scan_ok && h->shards == 1 && !opt.profile && opt.mid_loop >= 0 && (fits || opt.mid_loop > 0);
    }
    // overlapped graphs (build_graph), on request only: the idea -- on large trees the permutation outlasts the reduced-cost
    // patch, so the next pricing could hide beside it -- loses to the cost of the two cross-queue edges per pivot
    // (netgen_8_14a 55 K -> 33 K pivots/s, 1 M / 16 M 26 K -> 22 K; profiles/r02_ab_overlapped_graph.txt)
    {
        const bool able = !h->bpl && h->rcached && !h->small && !h->mid && h->shards == 1 && !opt.profile && opt.rule != MCF_RULE_CANDIDATE_LIST;
        h->overlap = able && opt.overlap_update > 0;
        h->overlap_cfg = h->overlap;
    }
    // compressed Dantzig keys for the grid sweeps of the Dantzig / candidate-list rules (4 B per arc instead of 9)
    // They pay where a sweep reads the whole shard and is bandwidth-bound: full (non-incremental) sweeps of the Dantzig rule
    // from kIncrementalMinArcs arcs on (1 M / 16 M: sweep 24 -> 14 us).  Keeping the codes exact costs the reduced-cost patch a state
    // byte and a 4-byte store per patched arc (k_update +1..3 us per pivot), which a candidate-list handle (one sweep per ~33
    // pivots) or an incremental sweep (1 % of the arcs re-read per pivot) never earns back.  compressed_keys: 1 = on, -1 = off.
    const bool keys_auto = opt.rule == MCF_RULE_DANTZIG_FULL && opt.full_sweeps > 0 && im.m >= kIncrementalMinArcs;
    h->want_vkey = h->rcached && !h->mid && opt.rule != MCF_RULE_DEVEX_BLOCK && h->key_mode == MCF_KEY_PLAIN &&
                   (opt.compressed_keys > 0 || (opt.compressed_keys == 0 && keys_auto));
    if (h->want_vkey) {
        const char* nt_env = std::getenv("MCF_NT_SWEEP");   // A/B switch: 0 / 1 force, unset = by size
        h->nt_sweep = nt_env ? nt_env[0] == '1' : (im.m_pad / (h->shards > 0 ? h->shards : 1)) * 4 > (int64_t)200 * 1024 * 1024;
    }
    // incremental pricing for the rules whose sweeps cover the whole shard (Dantzig, candidate list); not for the
    // persistent loop, whose instances are far too small for it (its kernel compiles the marking away)
    // (auto: only where a sweep is a large part of a pivot -- below ~4 M arcs the flag look-up in front of every
    // sweep and the marking in k_update cost more than the skipped blocks save: netgen_8_14a 52.7 K -> 46.7 K pivots/s;
    // at 16 M arcs: 23.9 K -> 37 K)
    h->want_dirty = h->rcached && !h->mid && opt.rule != MCF_RULE_DEVEX_BLOCK && (opt.full_sweeps < 0 || (opt.full_sweeps == 0 && im.m >= kIncrementalMinArcs));
    // candidate cache: the grid path of the candidate-list rule on one GPU, keys that need nothing but the reduced cost
    h->want_candx = opt.rule == MCF_RULE_CANDIDATE_LIST && h->shards == 1 && !h->small && !h->mid && !opt.profile && h->key_mode <= MCF_KEY_FORWARD_FIRST &&
                    h->price_blocks <= 2 * kPivotThreads && !std::getenv("MCF_NO_CANDX");
    // pivots back to back (k_pivot_run): candidate-list handles on the blocked list that keep the candidate cache
    h->run_pairs_cfg = 0;
    // Opt-in: measured at 1M/16M (first 300 K pivots, same box) 30.9-35.7 K pivots/s in the run shape against 41.1 K in the
    // pivot+update pair shape -- one workgroup's phase A over 8-20 K blocks costs more than the launches it saves.
    const char* run_env = std::getenv("MCF_PIVOT_RUN");
    const int want_run = opt.pivot_run > 0 ? opt.pivot_run : (run_env ? std::atoi(run_env) : 0);
    if (h->bpl && h->want_candx && want_run > 0 && opt.use_graph && !std::getenv("MCF_NO_RUN")) h->run_pairs_cfg = want_run;
    h->run_pairs = h->run_pairs_cfg;
    {
        // auto: candidate lists (one sweep per ~33 pivots) on large instances (from 100 000 nodes: measured at 1 M / 16 M) from an
        // average |T2| of 384 nodes, Devex there from 1 500; never for the Dantzig rule, whose every pivot sweeps all arcs, for
        // shards (their driver owns the launches) or the persistent loops.  rc_drop: -1 = never, k > 0 = that threshold.
        int64_t thr = 0;
        if (h->rcached && !h->mid && !h->small && h->shards == 1 && opt.key_mode == 0 && !opt.forward_first) {
            if (opt.rc_drop > 0) thr = opt.rc_drop;
            else if (opt.rc_drop == 0 && im.n_nodes >= 100000)
                // (Devex block search sweeps one block per pivot: the dearer sweep is paid every time, so it waits for larger
                //  subtrees -- 1 M / 16 M: 139.8 s without, 134.0 / 134.8 s with a threshold of 1 500 / 384)
                thr = opt.rule == MCF_RULE_CANDIDATE_LIST ? 384 : (opt.rule == MCF_RULE_DEVEX_BLOCK ? 1500 : 0);
            if (opt.rule == MCF_RULE_DANTZIG_FULL) thr = 0;
        }
        if (const char* env = std::getenv("MCF_RC_DROP")) { const long vv = std::atol(env); thr = vv > 0 ? vv : 0; }   // A/B switch
        h->rc_drop_subtree = h->rcached && h->shards == 1 ? thr : 0;
    }
}

// the geometry of `src` as it stands (mcf_add_arcs keeps the pricing grid and grows the LDS plan), for a handle of its image
void inherit_geometry(mcf_handle* h, const mcf_handle* src) {
    h->bpl = src->bpl; h->bpl_shift = src->bpl_shift; h->bpl_cap = src->bpl_cap; h->bpl_dense = src->bpl_dense; h->bpl_grid = src->bpl_grid;
    h->price_blocks = src->price_blocks; h->apply_blocks = src->apply_blocks; h->rcupd_blocks = src->rcupd_blocks;
    h->stream_owned = h->im.n > kPooledMaxNodes;
    h->key_mode = src->key_mode;
    h->small = src->small; h->small_threads = src->small_threads; h->small_narrow_ok = src->small_narrow_ok; h->small_layout = src->small_layout;
    h->scan_ok = src->scan_ok; h->climb_budget = src->climb_budget;
    h->rc_able = src->rc_able; h->rcached = src->rc_able; h->rc_partial = src->rc_partial;
    h->mid = src->mid;
    h->overlap_cfg = src->overlap_cfg; h->overlap = src->overlap_cfg;
    h->want_vkey = src->want_vkey; h->nt_sweep = src->nt_sweep; h->want_dirty = src->want_dirty; h->want_candx = src->want_candx;
    h->run_pairs_cfg = src->run_pairs_cfg; h->run_pairs = src->run_pairs_cfg;
    h->rc_drop_subtree = src->rc_drop_subtree;
}

template <typename T>
hipError_t take(mcf_handle* h, T** field, size_t count, const char* name, bool state) {
    const hipError_t e = dalloc(field, count);
    if (e == hipSuccess) h->arrays.push_back({reinterpret_cast<void**>(field), count * sizeof(T), state, name});
    return e;
}

// a handle that captures graphs needs a stream nobody else captures on: only the persistent-loop paths that launch plain
// kernels keep a borrowed stream
hipError_t own_stream_if_captured(mcf_handle* h) {
    if (h->stream_owned || h->small || (h->mid && h->opt.rule != MCF_RULE_CANDIDATE_LIST)) return hipSuccess;
    hipStream_t own = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&own, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    h->stream = own;
    h->stream_owned = true;
    return hipSuccess;
}

// Part two.  from_image: mcf_create -- the arrays that never change after creation (adjacency, priorities, the header of the
// incremental sweeps) are filled from the host and the ones a kernel may read before it writes are cleared; otherwise
// (mcf_fork) the device copy fills every state array.  State arrays (copied by a fork) and scratch are told apart here:
// scratch is what every pivot writes before it reads -- the two cycle sides and their records (path, ppos, rec), the
// permutation's segment table (seg) and the list of shrunken subtrees (chg) are written by the pivot's walk / finish and
// consumed by the same pivot's update; cand_aux and one are the buffers of mcf_price_once and the read-back of one candidate.
// On failure the caller frees the handle (free_all); *what names the step.
hipError_t alloc_wire(mcf_handle* h, bool from_image, const char** what) {
    const McfHostImage& im = h->im;
    const mcf_options& opt = h->opt;
    hipError_t e;
#define ALLOC_TRY(step, expr) do { if ((e = (expr)) != hipSuccess) { *what = step; return e; } } while (0)
    ALLOC_TRY("hipStreamCreate", h->stream_owned ? hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) : pool_stream(h->device, &h->stream));
    const size_t N = im.n_nodes;
    const bool S = true, X = false;   // state / scratch
    ALLOC_TRY("hipMalloc tail", take(h, &h->d_tail, im.m_pad, "tail", S));
    ALLOC_TRY("hipMalloc head", take(h, &h->d_head, im.m_pad, "head", S));
    ALLOC_TRY("hipMalloc cost", take(h, &h->d_cost, im.m_pad, "cost", S));
    ALLOC_TRY("hipMalloc orig", take(h, &h->d_orig, im.m_pad, "orig", S));
    ALLOC_TRY("hipMalloc state", take(h, &h->d_state, im.m_pad, "state", S));
    ALLOC_TRY("hipMalloc weight", take(h, &h->d_weight, im.m_pad, "weight", S));
    ALLOC_TRY("hipMalloc arcw", take(h, &h->d_arcw, im.arcw.size(), "arcw", S));
    ALLOC_TRY("hipMalloc pi", take(h, &h->d_pi, N, "pi", S));
    ALLOC_TRY("hipMalloc node", take(h, &h->d_node, N, "node", S));
    const size_t bpl_slots = h->bpl ? ((size_t)h->bpl_cap << h->bpl_shift) + 4 : 0;   // slots per arena (+4: groups of four)
    // (+4: the cycle scan reads the nodes in aligned groups of four, like the sizes)
    ALLOC_TRY("hipMalloc order", take(h, &h->d_order0, h->bpl ? bpl_slots : N + 4, "order0", S));
    ALLOC_TRY("hipMalloc order", take(h, &h->d_order1, h->bpl ? bpl_slots : N + 4, "order1", S));
    ALLOC_TRY("hipMalloc pos", take(h, &h->d_pos0, N, "pos0", S));
    ALLOC_TRY("hipMalloc pos", take(h, &h->d_pos1, h->bpl ? 1 : N, "pos1", S));
    ALLOC_TRY("hipMalloc path", take(h, &h->d_path1, N, "path1", X));
    ALLOC_TRY("hipMalloc path", take(h, &h->d_path2, N, "path2", X));
    ALLOC_TRY("hipMalloc path", take(h, &h->d_ppos1, h->bpl ? 2 * N : N, "ppos1", X));   // (blocked list: positions, then slots)
    ALLOC_TRY("hipMalloc path", take(h, &h->d_ppos2, h->bpl ? 2 * N : N, "ppos2", X));
    ALLOC_TRY("hipMalloc rec", take(h, &h->d_rec1, N, "rec1", X));
    ALLOC_TRY("hipMalloc rec", take(h, &h->d_rec2, N, "rec2", X));
    ALLOC_TRY("hipMalloc seg", take(h, &h->d_seg, 2 * N + 2, "seg", X));
    ALLOC_TRY("hipMalloc ctx", take(h, &h->d_ctx, 1, "ctx", S));
    ALLOC_TRY("hipMalloc cand", take(h, &h->d_cand, kMaxPriceBlocks, "cand", S));
    ALLOC_TRY("hipMalloc cand", take(h, &h->d_cand_aux, kMaxPriceBlocks, "cand_aux", X));
    if (from_image) ALLOC_TRY("hipMemset cand", hipMemset(h->d_cand, 0xff, kMaxPriceBlocks * sizeof(McfCand)));
    ALLOC_TRY("hipMalloc one", take(h, &h->d_one, 1, "one", X));
    ALLOC_TRY("hipMalloc swept", take(h, &h->d_swept, kMaxPriceBlocks, "swept", S));
    {   // pinned: the control block's host copy and the one-candidate read-back buffer (one pooled slot)
        char* slot = nullptr;
        ALLOC_TRY("hipHostMalloc", pinned_take(&slot));
        h->h_ctx = reinterpret_cast<McfCtx*>(slot);
        h->h_one = reinterpret_cast<McfCand*>(slot + ((sizeof(McfCtx) + 63) & ~(size_t)63));
    }

    McfView& v = h->view;
    v.n_nodes = im.n_nodes;
    v.m = im.m;
    v.tail = h->d_tail; v.head = h->d_head; v.cost = h->d_cost; v.orig = h->d_orig; v.state = h->d_state;
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) v.bucket_off[x] = im.bucket_off[x];
    v.weight = opt.rule == MCF_RULE_DEVEX_BLOCK ? h->d_weight : nullptr;
    v.dx = nullptr;
    if (opt.rule == MCF_RULE_DEVEX_BLOCK) {   // granule table + touched-weight list (the table is filled by upload_image, once)
        ALLOC_TRY("hipMalloc granule table", take(h, &h->d_dx, 1, "devex", S));
        v.dx = h->d_dx;
    }
    // key variant of the Dantzig / candidate-list sweep (the reference's specialised entering rules, mcf_core.h: mcf_dantzig_key)
    v.key_mode = h->key_mode;
    v.prio = nullptr;
    if (v.key_mode == MCF_KEY_PRIORITY) {
        ALLOC_TRY("hipMalloc priority", take(h, &h->d_prio, im.m_pad, "priority", S));
        if (from_image) {
            std::vector<int8_t> pr((size_t)im.m_pad, 0);   // the caller's order -> engine order
            for (int64_t i = 0; i < im.m; ++i) pr[(size_t)i] = (int8_t)(opt.arc_priority[im.orig[(size_t)i]] & 3);
            ALLOC_TRY("hipMemcpy priority", hipMemcpy(h->d_prio, pr.data(), pr.size(), hipMemcpyHostToDevice));
        }
        v.prio = h->d_prio;
    }
    v.arcw = h->d_arcw; v.pi = h->d_pi; v.node = h->d_node;
    v.order[0] = h->d_order0; v.order[1] = h->d_order1;
    v.posbuf[0] = h->d_pos0; v.posbuf[1] = h->d_pos1;
    v.psz[0] = nullptr; v.psz[1] = nullptr;
    v.reach = nullptr; v.chg = nullptr;
    v.path1 = h->d_path1; v.path2 = h->d_path2; v.ppos1 = h->d_ppos1; v.ppos2 = h->d_ppos2; v.rec1 = h->d_rec1; v.rec2 = h->d_rec2; v.seg = h->d_seg; v.ctx = h->d_ctx;

    v.bmeta[0] = v.bmeta[1] = nullptr; v.bext[0] = v.bext[1] = nullptr; v.blk_shift = 0; v.blk_cap = 0; v.ncandx = 0; v.candx = nullptr;
    if (h->bpl) {
        // the two slot arenas (sizes; node ids are d_order0/1), the block records (two copies) and extents (one per arena),
        // and the scratch the scan spills flagged blocks to
        ALLOC_TRY("hipMalloc psz", take(h, &h->d_psz0, bpl_slots, "psz0", S));
        ALLOC_TRY("hipMalloc psz", take(h, &h->d_psz1, bpl_slots, "psz1", S));
        if (from_image) { ALLOC_TRY("hipMemset psz", hipMemset(h->d_psz0, 0, bpl_slots * 4)); ALLOC_TRY("hipMemset psz", hipMemset(h->d_psz1, 0, bpl_slots * 4)); }
        for (int a = 0; a < 2; ++a) {
            ALLOC_TRY("hipMalloc block records", take(h, &h->d_bmeta[a], (size_t)h->bpl_cap + 2, a ? "bmeta1" : "bmeta0", S));
            ALLOC_TRY("hipMalloc block extents", take(h, &h->d_bext[a], (size_t)h->bpl_cap, a ? "bext1" : "bext0", S));
            v.bmeta[a] = h->d_bmeta[a]; v.bext[a] = h->d_bext[a];
        }
        const size_t nchg = std::max(N, 2 * (size_t)h->bpl_cap + 2);
        ALLOC_TRY("hipMalloc chg", take(h, &h->d_chg, nchg, "chg", X));
        v.psz[0] = h->d_psz0; v.psz[1] = h->d_psz1;
        v.chg = h->d_chg;
        v.blk_shift = h->bpl_shift; v.blk_cap = h->bpl_cap;
    } else if (h->scan_ok) {
        const size_t NP = (N + MCF_REACH_BLOCK - 1) / MCF_REACH_BLOCK * MCF_REACH_BLOCK + 4;  // whole coarse blocks (+4: groups of four)
        ALLOC_TRY("hipMalloc psz", take(h, &h->d_psz0, NP, "psz0", S));
        ALLOC_TRY("hipMalloc psz", take(h, &h->d_psz1, NP, "psz1", S));
        if (from_image) { ALLOC_TRY("hipMemset psz", hipMemset(h->d_psz0, 0, NP * 4)); ALLOC_TRY("hipMemset psz", hipMemset(h->d_psz1, 0, NP * 4)); }
        v.psz[0] = h->d_psz0; v.psz[1] = h->d_psz1;
        ALLOC_TRY("hipMalloc reach", take(h, &h->d_reach, NP / MCF_REACH_BLOCK + 8, "reach", S));   // (+8: read four at a time)
        if (from_image) ALLOC_TRY("hipMemset reach", hipMemset(h->d_reach, 0, (NP / MCF_REACH_BLOCK + 8) * 4));
        ALLOC_TRY("hipMalloc chg", take(h, &h->d_chg, N, "chg", X));
        v.reach = h->d_reach; v.chg = h->d_chg;
    }
    if (h->rc_able) {
        if (from_image) mcf_build_rcache(h->im, h->rc_partial ? h->shard : 0, h->rc_partial ? h->shards : 1);
        v.rc_partial = h->rc_partial ? 1 : 0;
        ALLOC_TRY("hipMalloc rcache", take(h, &h->d_rcache, im.m_pad, "rcache", S));
        ALLOC_TRY("hipMalloc adj_off", take(h, &h->d_adj_off, im.adj_off.size(), "adj_off", S));
        // (the image gives its adjacency up once it is on the device: its length is 2 m either way)
        ALLOC_TRY("hipMalloc adj", take(h, &h->d_adj, from_image ? im.adj.size() : (size_t)(2 * im.m), "adj", S));
        if (from_image) {
            ALLOC_TRY("copy adj_off", hipMemcpy(h->d_adj_off, im.adj_off.data(), im.adj_off.size() * 8, hipMemcpyHostToDevice));
            ALLOC_TRY("copy adj", hipMemcpy(h->d_adj, im.adj.data(), im.adj.size() * 8, hipMemcpyHostToDevice));
            h->im.adj.clear(); h->im.adj.shrink_to_fit();  // the device copy is the only one needed from here on
        }
        v.rcache = h->d_rcache; v.adj_off = h->d_adj_off; v.adj = h->d_adj;
    } else {
        v.rcache = nullptr; v.adj_off = nullptr; v.adj = nullptr; v.rc_partial = 0;
    }
    if (h->overlap_cfg) ALLOC_TRY("hipStreamCreate", hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    v.vkey = nullptr;
    v.vk_bigm = im.big_m;
    v.vk_half = 1 << (opt.vkey_half_log2 > 0 && opt.vkey_half_log2 <= 28 ? opt.vkey_half_log2 : 28);
    if (h->want_vkey) {
        ALLOC_TRY("hipMalloc vkey", take(h, &h->d_vkey, im.m_pad, "vkey", S));
        v.vkey = h->d_vkey;
    }
    v.dirty = nullptr;
    if (h->want_dirty) {
        static_assert(MCF_MAX_PRICE_BLOCKS == kMaxPriceBlocks, "flag array size");
        ALLOC_TRY("hipMalloc dirty", take(h, &h->d_dirty, 1, "dirty", S));
        if (from_image) {
            McfDirty head;  // (the flags are raised by upload_image)
            head.nlb = h->price_blocks / MCF_NUM_BUCKETS;
            for (int x = 0; x < MCF_NUM_BUCKETS; ++x) {
                int64_t lo, hi;
                mcf_bucket_slice(im.bucket_off, x, h->shard, h->shards, 0, 1, &lo, &hi);
                head.lo[x] = (int32_t)lo; head.hi[x] = (int32_t)hi;
            }
            ALLOC_TRY("copy dirty", hipMemcpy(h->d_dirty, &head, offsetof(McfDirty, flag), hipMemcpyHostToDevice));
        }
        v.dirty = h->d_dirty;
    }
    v.candx = nullptr; v.ncandx = 0;
    if (h->want_candx) {
        ALLOC_TRY("hipMalloc candidate records", take(h, &h->d_candx, kMaxPriceBlocks, "candx", S));
        if (from_image) ALLOC_TRY("hipMemset candidate records", hipMemset(h->d_candx, 0xff, kMaxPriceBlocks * sizeof(McfCandX)));
        v.candx = h->d_candx; v.ncandx = h->price_blocks;
    }
#undef ALLOC_TRY
    return hipSuccess;
}

}  // namespace

#include "mcf_passes_host.h"

// ====================================================================== mcf_fork / mcf_restore (include/mcf.h)
namespace {

// The host half of a fork: every field of the handle a later call reads and that is state, not geometry.  (The image is
// assigned by the caller: a fork needs it before it allocates.)  Captured graphs are not copied -- they carry the view by
// value -- and neither is the scratch of the post-solve passes, nor the index mcf_update_costs builds on first use.
void fork_host_state(mcf_handle* f, const mcf_handle* src) {
    *f->h_ctx = *src->h_ctx;
    f->ctx_current = true;
    f->external_driver = src->external_driver;
    f->stats = src->stats;
    f->total_cap = src->total_cap;
    f->solved_once = src->solved_once;
    f->run_pairs = src->run_pairs; f->run_low = src->run_low; f->run_seen = src->run_seen;
    f->rc_dropped = src->rc_dropped; f->rcached = src->rcached; f->overlap = src->overlap;
    f->sw_pivots = src->sw_pivots; f->sw_subtree = src->sw_subtree;
    f->shard_arcs = src->shard_arcs; f->priced_per_pass = src->priced_per_pass;
    f->dx_filled = f->d_dx != nullptr;
    McfView& v = f->view;
    v.n_nodes = f->im.n_nodes; v.m = f->im.m;
    for (int x = 0; x <= MCF_NUM_BUCKETS; ++x) v.bucket_off[x] = f->im.bucket_off[x];
    v.vk_bigm = src->view.vk_bigm; v.vk_half = src->view.vk_half;
    // a handle that dropped its reduced costs keeps the arrays and prices from the potentials (mcf_solve)
    v.rcache = src->rc_dropped || !f->rc_able ? nullptr : f->d_rcache;
    v.vkey = src->rc_dropped ? nullptr : f->d_vkey;
    v.dirty = src->rc_dropped ? nullptr : f->d_dirty;
    f->uc_inv.clear(); f->uc_stamp.clear();
}

// The device half: one launch of k_fork over the state arrays of `src` into the `count` handles of dst (same geometry: their
// array lists were made by the same alloc_wire).  MCF_FORK_MEMCPY=1 (A/B switch, read at the call): one hipMemcpyAsync per
// array and destination instead.  MCF_FORK_NT = 0 / 1 forces plain / non-temporal stores (default: by the size of a fork).
int fork_device_copy(mcf_handle* src, mcf_handle* const* dst, int32_t count, mcf_fork_report* rep) {
    std::vector<McfForkSeg> segs;
    int64_t chunks = 0, bytes = 0;
    for (const mcf_handle::DevArray& a : src->arrays) {
        if (!a.state) continue;
        McfForkSeg sg;
        sg.src = static_cast<const char*>(*a.field); sg.bytes = (int64_t)a.bytes; sg.chunk0 = chunks; sg.slot = (int32_t)segs.size(); sg.pad = 0;
        chunks += mcf_fork_chunks(sg.bytes);
        bytes += sg.bytes;
        segs.push_back(sg);
    }
    const size_t nseg = segs.size();
    std::vector<char*> table((size_t)count * nseg);
    for (int32_t d = 0; d < count; ++d) {
        size_t slot = 0;
        for (const mcf_handle::DevArray& a : dst[d]->arrays) {
            if (!a.state) continue;
            if (slot >= nseg || (int64_t)a.bytes != segs[slot].bytes) { src->err = "internal: array lists of a fork differ"; return MCF_E_INTERNAL; }
            table[(size_t)d * nseg + slot++] = static_cast<char*>(*a.field);
        }
        if (slot != nseg) { src->err = "internal: array lists of a fork differ"; return MCF_E_INTERNAL; }
    }
    hipStream_t s = src->stream;
    hipEvent_t ev[2] = {nullptr, nullptr};
    char* d_tab = nullptr;
    const size_t seg_bytes = (nseg * sizeof(McfForkSeg) + 15) & ~(size_t)15, tab_bytes = table.size() * sizeof(char*);
    auto done = [&](int code, const char* what) {
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        (void)hipFree(d_tab);
        if (code != MCF_OK) { (void)hipGetLastError(); src->err = what; }
        return code;
    };
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) return done(MCF_E_HIP, "hipEventCreate");
    const char* mc = std::getenv("MCF_FORK_MEMCPY");
    const bool by_memcpy = mc && mc[0] == '1';
    if (!by_memcpy) {
        if (hipMalloc(reinterpret_cast<void**>(&d_tab), seg_bytes + tab_bytes + 16) != hipSuccess) return done(MCF_E_ALLOC, "hipMalloc of the copy's segment table");
        if (hipMemcpyAsync(d_tab, segs.data(), nseg * sizeof(McfForkSeg), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(d_tab + seg_bytes, table.data(), tab_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)   // (pageable sources)
            return done(MCF_E_HIP, "upload of the copy's segment table");
    }
    if (hipEventRecord(ev[0], s) != hipSuccess) return done(MCF_E_HIP, "hipEventRecord");
    if (by_memcpy) {
        for (int32_t d = 0; d < count; ++d)
            for (size_t i = 0; i < nseg; ++i)
                if (segs[i].bytes > 0 && hipMemcpyAsync(table[(size_t)d * nseg + i], segs[i].src, (size_t)segs[i].bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
                    return done(MCF_E_HIP, "hipMemcpyAsync of an array");
    } else if (chunks > 0) {
        // Store flavour, as measured on MI355X (profiles/fork_scenarios.txt): a fork of 152 MB -- source plus destination
        // larger than the Infinity Cache -- takes 0.067 ms with non-temporal stores against 0.071 ms with plain ones; the
        // small forks of a scenario batch are read again at once by their edits and solves and keep plain stores.
        const char* nt_env = std::getenv("MCF_FORK_NT");
        const bool nt = nt_env ? nt_env[0] == '1' : bytes > ((int64_t)128 << 20);
        const int64_t items = mcf_fork_items(chunks, count);
        const unsigned grid = (unsigned)(items < 2048 ? items : 2048);   // 8 workgroups per CU; the rest by the grid-stride loop
        const McfForkSeg* d_seg = reinterpret_cast<const McfForkSeg*>(d_tab);
        char* const* d_dst = reinterpret_cast<char* const*>(d_tab + seg_bytes);
        if (nt) hipLaunchKernelGGL(k_fork<true>, dim3(grid), dim3(MCF_FORK_THREADS), 0, s, d_seg, (int32_t)nseg, chunks, d_dst, (int64_t)count);
        else hipLaunchKernelGGL(k_fork<false>, dim3(grid), dim3(MCF_FORK_THREADS), 0, s, d_seg, (int32_t)nseg, chunks, d_dst, (int64_t)count);
        if (hipGetLastError() != hipSuccess) return done(MCF_E_HIP, "launch of the copy kernel");
    }
    if (hipEventRecord(ev[1], s) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess) return done(MCF_E_HIP, "the device copy failed");
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
    if (rep) { rep->count = count; rep->segments = (int64_t)nseg; rep->bytes_per_fork = bytes; rep->device_ms = ms; }
    return done(MCF_OK, "");
}

int fork_check_src(mcf_handle* src, const char* who) {
    if (src->shards != 1) {
        src->err = std::string(who) + ": handle was created with shard_count > 1; sharded handles cannot be forked";
        return MCF_E_STATE;
    }
    HIP_TRY(src, hipSetDevice(src->device));
    HIP_TRY(src, hipStreamSynchronize(src->stream));
    return sync_ctx(src, src->stream);   // (reads the control block; writes nothing the solver reads)
}

}  // namespace

int mcf_fork(mcf_handle* src, int32_t count, mcf_handle** out, mcf_fork_report* report) {
    if (!src || !out || count < 0) { g_create_error = "mcf_fork: null src / out or count < 0"; if (src) src->err = g_create_error; return MCF_E_BAD_ARG; }
    if (report) std::memset(report, 0, sizeof *report);
    if (count == 0) return MCF_OK;
    for (int32_t i = 0; i < count; ++i) out[i] = nullptr;
    int rc = fork_check_src(src, "mcf_fork");
    if (rc) { g_create_error = src->err; return rc; }
    auto undo = [&](int code, const std::string& msg) {
        for (int32_t i = 0; i < count; ++i) if (out[i]) { free_all(out[i]); delete out[i]; out[i] = nullptr; }
        (void)hipGetLastError();
        g_create_error = msg; src->err = msg;
        return code;
    };
    for (int32_t i = 0; i < count; ++i) {
        mcf_handle* f = new (std::nothrow) mcf_handle();
        if (!f) return undo(MCF_E_ALLOC, "mcf_fork: host allocation");
        out[i] = f;
        try { f->im = src->im; } catch (const std::bad_alloc&) { return undo(MCF_E_ALLOC, "mcf_fork: host allocation of the image"); }
        f->opt = src->opt;
        f->opt.arc_priority = nullptr;   // (the source's pointer was only valid during mcf_create)
        f->device = src->device;
        f->shards = src->shards; f->shard = src->shard;
        inherit_geometry(f, src);
        const char* what = "";
        const hipError_t e = alloc_wire(f, false, &what);
        if (e != hipSuccess) return undo(e == hipErrorOutOfMemory ? MCF_E_ALLOC : MCF_E_HIP, std::string("mcf_fork: ") + what + ": " + hipGetErrorString(e));
        if (own_stream_if_captured(f) != hipSuccess) return undo(MCF_E_HIP, "mcf_fork: hipStreamCreate");
        fork_host_state(f, src);
        f->shape = src->shape;
    }
    rc = fork_device_copy(src, out, count, report);
    if (rc) return undo(rc, "mcf_fork: " + src->err);
    return MCF_OK;
}

int mcf_restore(mcf_handle* const* dst, int32_t count, mcf_handle* src, mcf_fork_report* report) {
    if (!src || !dst || count < 0) { if (src) src->err = "mcf_restore: null dst or count < 0"; return MCF_E_BAD_ARG; }
    if (report) std::memset(report, 0, sizeof *report);
    for (int32_t i = 0; i < count; ++i) {
        if (!dst[i] || dst[i] == src) { src->err = "mcf_restore: a destination is null or the source itself"; return MCF_E_BAD_ARG; }
        for (int32_t j = 0; j < i; ++j) if (dst[j] == dst[i]) { src->err = "mcf_restore: a destination is named twice"; return MCF_E_BAD_ARG; }
    }
    if (count == 0) return MCF_OK;
    if (src->shards != 1) { src->err = "mcf_restore: handle was created with shard_count > 1; sharded handles cannot be forked"; return MCF_E_STATE; }
    for (int32_t i = 0; i < count; ++i) {
        const mcf_handle* d = dst[i];
        const char* field = nullptr;
        for (size_t k = 0; k < src->shape.size() && !field; ++k)
            if (d->shape.size() != src->shape.size() || d->shape[k].second != src->shape[k].second) field = src->shape[k].first;
        for (size_t k = 0; k < src->arrays.size() && !field; ++k)
            if (d->arrays.size() != src->arrays.size() || d->arrays[k].bytes != src->arrays[k].bytes) field = src->arrays[k].name;
        if (field) {
            src->err = "mcf_restore: destination " + std::to_string(i) + " has another shape than the source: " + field;
            return MCF_E_STATE;
        }
    }
    int rc = fork_check_src(src, "mcf_restore");
    if (rc) return rc;
    for (int32_t i = 0; i < count; ++i) {   // host allocation first: nothing has changed if it fails
        try { dst[i]->im = src->im; } catch (const std::bad_alloc&) { src->err = "mcf_restore: host allocation of the image"; return MCF_E_ALLOC; }
    }
    for (int32_t i = 0; i < count; ++i) HIP_TRY(src, hipStreamSynchronize(dst[i]->stream));
    rc = fork_device_copy(src, dst, count, report);
    if (rc) return rc;
    for (int32_t i = 0; i < count; ++i) {
        mcf_handle* f = dst[i];
        f->opt = src->opt;
        f->opt.arc_priority = nullptr;
        f->climb_budget = src->climb_budget; f->rc_drop_subtree = src->rc_drop_subtree; f->run_pairs_cfg = src->run_pairs_cfg;
        f->small_layout = src->small_layout; f->small_narrow_ok = src->small_narrow_ok; f->nt_sweep = src->nt_sweep;
        fork_host_state(f, src);
        drop_graph(f);   // (rebuilt on first use)
        // scratch of the post-solve passes that caches the instance: filled again on first use
        lazy_release({{&f->d_ct_supply, 0}, {&f->d_ct_adj_off, 0}, {&f->d_ct_adj, 0}});
        f->err.clear();
    }
    return MCF_OK;
}

// ====================================================================== C ABI
extern "C" {

int mcf_abi_version(void) { return MCF_ABI_VERSION; }

int mcf_small_narrow_ok(int64_t big_m, int64_t max_abs_cost, int64_t* bound) {
    if (bound) *bound = mcf_small_rc_bound(big_m, max_abs_cost);
    return mcf_small_narrow_fits(big_m, max_abs_cost) ? 1 : 0;
}

int mcf_device_count(void) { return usable_devices(); }

void mcf_default_options(mcf_options* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof *opt);
    opt->abi_version = MCF_ABI_VERSION;
    opt->device = -1;
    opt->rule = MCF_RULE_DANTZIG_FULL;
    opt->batch_pivots = 64;
    opt->use_graph = 1;
}

const char* mcf_last_error(mcf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int mcf_create(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
               const int64_t* supply, const mcf_options* opt_in, mcf_handle** out) {
    if (!out) return MCF_E_BAD_ARG;
    *out = nullptr;
    mcf_options opt;
    if (opt_in) opt = *opt_in; else mcf_default_options(&opt);
    if (opt.abi_version != MCF_ABI_VERSION) { g_create_error = "mcf_options.abi_version mismatch"; return MCF_E_BAD_ARG; }
    if (opt.key_mode < 0 || opt.key_mode > MCF_KEY_CAPACITY || (opt.key_mode == MCF_KEY_PRIORITY && !opt.arc_priority) ||
        (opt.key_mode > 0 && opt.rule == MCF_RULE_DEVEX_BLOCK)) {
        g_create_error = "mcf_options.key_mode: 0..3, MCF_KEY_PRIORITY needs arc_priority, and the key variants belong to the Dantzig / candidate-list rules";
        return MCF_E_BAD_ARG;
    }
    if (opt.rule != MCF_RULE_DANTZIG_FULL && opt.rule != MCF_RULE_DEVEX_BLOCK && opt.rule != MCF_RULE_CANDIDATE_LIST) {
        g_create_error = "unknown pricing rule";
        return MCF_E_BAD_ARG;
    }
    const int ndev = usable_devices();
    if (ndev <= 0) { g_create_error = "no HIP device available (the engine has no CPU path)"; return MCF_E_NO_DEVICE; }
    mcf_handle* h = new (std::nothrow) mcf_handle();
    if (!h) return MCF_E_ALLOC;
    int err = 0;
    const std::string msg = mcf_build_image(n, m, tail, head, cost, cap, supply, h->im, &err);
    if (err) { g_create_error = msg; delete h; return err; }
    h->opt = opt;
    if (h->opt.batch_pivots <= 0) h->opt.batch_pivots = 64;
    if (opt.device >= 0) {
        if (opt.device >= ndev) { g_create_error = "device ordinal out of range"; delete h; return MCF_E_BAD_ARG; }
        if (hipSetDevice(opt.device) != hipSuccess) { g_create_error = "hipSetDevice failed"; delete h; return MCF_E_HIP; }
    }
    if (hipGetDevice(&h->device) != hipSuccess) { g_create_error = "hipGetDevice failed"; delete h; return MCF_E_HIP; }
    // shard
    h->shards = opt.shard_count > 0 ? opt.shard_count : 1;
    h->shard = opt.shard_rank;
    if (h->shard < 0 || h->shard >= h->shards) {
        g_create_error = "bad shard_rank / shard_count";
        delete h;
        return MCF_E_BAD_ARG;
    }
    decide_geometry(h);
    const char* what = "";
    hipError_t e = alloc_wire(h, true, &what);
    auto fail = [&](const char* step, hipError_t err) {
        g_create_error = std::string(step) + ": " + hipGetErrorString(err);
        free_all(h);
        delete h;
        return err == hipErrorOutOfMemory ? MCF_E_ALLOC : MCF_E_HIP;
    };
    if (e != hipSuccess) return fail(what, e);
    const int rc = upload_image(h);   // (ends with a synchronisation of h->stream)
    if (rc != MCF_OK) { g_create_error = h->err; free_all(h); delete h; return rc; }
    if ((e = own_stream_if_captured(h)) != hipSuccess) return fail("hipStreamCreate", e);
    h->shape = shape_of(h);
    *out = h;
    return MCF_OK;
}

int mcf_reset(mcf_handle* h) {
    if (!h) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    mcf_init_cold_basis(h->im);  // a warm start may have replaced the start basis in the host image
    mcf_refresh_rcache(h->im);
    return upload_image(h);
}

int mcf_set_basis(mcf_handle* h, const int8_t* in_tree, const int8_t* at_upper) {
    if (!h || !in_tree) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    const std::string msg = mcf_apply_basis(h->im, in_tree, at_upper);
    if (!msg.empty()) mcf_init_cold_basis(h->im);  // rejected: the image may be half written
    mcf_refresh_rcache(h->im);
    const int rc = upload_image(h);
    if (rc) return rc;
    if (!msg.empty()) { h->err = "warm-start basis rejected: " + msg; return MCF_E_STATE; }
    return MCF_OK;
}

int mcf_set_max_pivots(mcf_handle* h, int64_t max_total_pivots) {
    if (!h) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_ctl, dim3(1), dim3(1), 0, h->stream, h->d_ctx, max_total_pivots, 1);
    HIP_TRY(h, hipGetLastError());
    // the caller enqueues the pivots on a stream of its own: make the new cap visible first
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->total_cap = max_total_pivots;
    h->ctx_current = false;
    h->external_driver = true;
    return MCF_OK;
}

int mcf_solve(mcf_handle* h, int64_t max_pivots, mcf_progress_cb cb, void* user, int64_t cb_interval) {
    if (!h) return MCF_E_BAD_ARG;
    if (h->shards != 1) {
        // a sharded handle prices 1/shard_count of the arcs: on its own it would declare "optimal" as soon as ITS share
        // holds no eligible arc.  It is only valid inside the price -> all-gather -> pivot protocol below.
        h->err = "mcf_solve: handle was created with shard_count > 1; drive it with mcf_enqueue_price / mcf_enqueue_pivot";
        return MCF_E_STATE;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t m = h->im.m, n = h->im.n;
    if (max_pivots < 0) max_pivots = 20 * (m + n) > 100 ? 20 * (m + n) : 100;  // simplex.py:1470
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    h->external_driver = false;   // from here on the library enqueues the pivots itself
    const int64_t start = h->h_ctx->pivots;
    const int64_t final_cap = start + max_pivots;
    if (cb_interval <= 0) cb_interval = 100;
    int batch = h->opt.batch_pivots;
    if (h->mid) {  // a slot is a whole run of pivots there
        const int per = h->opt.rule == MCF_RULE_CANDIDATE_LIST ? mcf_minor_cap(h->price_blocks) + 1 : batch;
        batch = batch / per > 2 ? batch / per : 2;
        if (h->opt.rule != MCF_RULE_CANDIDATE_LIST) batch = 1;
    }
    if (!h->mid && !h->small && h->opt.rule == MCF_RULE_CANDIDATE_LIST) {
        // The sweep cadence inside a batch is fixed (one sweep per minor_cap + 1 slots, launch_pivot_triplet): a batch that is
        // not a whole number of such periods leaves the next batch's first sweep slot in front of a list that is still
        // live, the sweep is skipped and the slots up to the following sweep slot idle (1 M / 16 M: 33 pivots per 64-slot
        // graph).  Whole periods only: 64 -> 66 slots at period 33, 63 at period 9.
        const int period = mcf_minor_cap(h->price_blocks) + 1;
        const int periods = (batch + period / 2) / period;
        batch = (periods > 0 ? periods : 1) * period;
    }
    const bool graph = h->opt.use_graph && !h->opt.profile && !h->small && !(h->mid && batch == 1);
    if (graph) { rc = build_graph(h, batch); if (rc) return rc; }
    bool stop = false;
    while (!stop) {
        // inner cap: stop at the next progress point so the callback cadence is exact
        int64_t cap = final_cap;
        if (cb) {
            const int64_t done = h->h_ctx->pivots - start;
            const int64_t next_cb = start + (done / cb_interval + 1) * cb_interval;
            if (next_cb < cap) cap = next_cb;
        }
        // the persistent loops outside a graph take the cap as a kernel argument; the other paths re-arm with k_ctl
        const bool arm_in_kernel = h->small || (h->mid && !graph && !h->opt.profile);
        if (!arm_in_kernel) hipLaunchKernelGGL(k_ctl, dim3(1), dim3(1), 0, h->stream, h->d_ctx, cap, 1);
        h->ctx_current = false;
        // pivot until the device reports something other than "still running"
        for (;;) {
            const bool timed_loop = arm_in_kernel;  // one kernel = many pivots: its duration is the per-launch figure bench.py reports
            if (timed_loop) {
                if (!h->loop_ev[0]) { HIP_TRY(h, hipEventCreate(&h->loop_ev[0])); HIP_TRY(h, hipEventCreate(&h->loop_ev[1])); }
                HIP_TRY(h, hipEventRecord(h->loop_ev[0], h->stream));
            }
            if (h->small) {
                const int32_t narrow = small_narrow_for(h->im, h->small_narrow_ok);   // (per launch: big-M may have grown)
                h->stats.small_narrow = narrow;
                const bool front = small_front_for(narrow, h->opt.rule, h->view.key_mode, h->view);
                hipLaunchKernelGGL(small_kernel(h->small_threads, front), dim3(1), dim3(h->small_threads == 1024 ? 1024 : 256), h->small_layout.total, h->stream, h->view,
                                   h->small_layout, h->opt.rule, h->d_cand, cap, h->h_ctx);
            }
            else {
                // eager launches need not run past the cap (a replayed graph has a fixed length: its surplus slots early-exit)
                const int64_t left = cap - h->h_ctx->pivots;
                const int slots = h->mid ? batch : (int)(left < 1 ? 1 : (left < batch ? left : batch));
                // a replayed graph has a fixed length: when fewer pivots than that are left (a small budget, the tail of a
                // progress interval) its surplus slots would idle through three early-exit kernels each -- launch just the slots
                // that are needed instead (bench.py --steps 20 on a 64-slot graph: 73 us per pivot, 41 us of them real)
                if (h->opt.profile) { rc = run_batch_profiled(h, slots); if (rc) return rc; }
                else if (graph && (h->mid || left >= batch)) HIP_TRY(h, hipGraphLaunch(h->graph_exec, h->stream));
                else for (int i = 0; i < slots; ++i) launch_pivot_triplet(h, h->stream, i, arm_in_kernel ? cap : (int64_t)-1);
            }
            if (timed_loop) HIP_TRY(h, hipEventRecord(h->loop_ev[1], h->stream));
            HIP_TRY(h, hipGetLastError());
            if (h->small) {   // the kernel wrote the host's pinned copy itself
                // (polling a pinned done word instead was tried: the wake-up saved here comes back in the caller's own
                //  device synchronisation, and a system-scope fence in front of the word cost 15 us of kernel time)
                HIP_TRY(h, hipStreamSynchronize(h->stream));
                h->ctx_current = true;
            } else {
                rc = read_ctx(h, h->stream);
                if (rc) return rc;
            }
            if (timed_loop) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, h->loop_ev[0], h->loop_ev[1]) == hipSuccess) { h->stats.loop_ms += ms; h->stats.loop_launches += 1; }
            }
            h->stats.batches += 1;
            if (h->h_ctx->status != MCF_RUNNING) break;
            // Run shape: still worth it?  A run launch that ends after a pivot or two (its update was too large for one
            // workgroup) is a k_pivot with extra baggage, and a period then needs more launches than the shape holds.  Three
            // batches in a row with fewer than three pivots per run launch: back to one k_pivot per slot, for good.
            if (h->run_pairs > 0 && graph) {
                const int period = mcf_minor_cap(h->price_blocks) + 1;
                const int64_t made = h->h_ctx->pivots - h->run_seen;
                h->run_seen = h->h_ctx->pivots;
                const int64_t launches = (int64_t)(batch / period) * h->run_pairs;
                h->run_low = made < 3 * launches ? h->run_low + 1 : 0;
                if (h->run_low >= 3) {
                    h->run_pairs = 0;
                    h->stats.run_left_at = h->h_ctx->pivots;
                    drop_graph(h);
                    rc = build_graph(h, batch);
                    if (rc) return rc;
                }
            }
            // Drop the resident reduced costs?  Their patch walks the adjacency of every node of the re-hung subtree: a few
            // arcs early in a solve, hundreds of thousands of random read-modify-writes per pivot once subtrees of thousands
            // of nodes move (1 M / 16 M, last third of the solve: 20+ us of a pivot).  Pricing from the potentials costs a
            // dearer sweep instead (gathers), which a candidate-list handle pays once per minor_cap + 1 pivots and a Devex
            // handle on one block.  Same keys, same candidates, same pivots; one way (until the next reset).
            if (h->rcached && h->rc_drop_subtree > 0 && !h->opt.profile) {
                const int64_t dp = h->h_ctx->pivots - h->sw_pivots, ds = h->h_ctx->subtree_nodes - h->sw_subtree;
                if (dp >= 4096) {
                    h->sw_pivots = h->h_ctx->pivots; h->sw_subtree = h->h_ctx->subtree_nodes;
                    if (ds >= dp * h->rc_drop_subtree) {
                        h->rc_dropped = true;
                        h->rcached = false;
                        h->overlap = false;   // (two-stream graphs price beside the permutation: only valid from resident values)
                        h->view.rcache = nullptr; h->view.vkey = nullptr; h->view.dirty = nullptr;
                        h->stats.rc_dropped_at = h->h_ctx->pivots;
                        if (graph) {
                            drop_graph(h);
                            rc = build_graph(h, batch);
                            if (rc) return rc;
                        }
                    }
                }
            }
        }
        const int32_t st = h->h_ctx->status;
        if (st == MCF_PIVOT_LIMIT && h->h_ctx->pivots < final_cap) {
            if (cb) {
                const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (cb(user, h->h_ctx->pivots, final_cap, el) != 0) stop = true;
            }
            continue;  // re-arm with the next cap
        }
        stop = true;
    }
    if (h->h_ctx->status == MCF_PIVOT_LIMIT && !h->h_ctx->limit_checked) {
        // simplex.py:1678-1699: at the budget, price once more to tell optimal from iteration_limit
        // (the persistent loops have done that on the device: limit_checked)
        int64_t arc = -1, key = 0; int32_t dir = 0;
        rc = mcf_price_once(h, h->opt.rule == MCF_RULE_DEVEX_BLOCK ? MCF_RULE_DANTZIG_FULL : h->opt.rule, 0, m, &arc, &dir, &key);
        if (rc) return rc;
        if (arc < 0) {
            h->h_ctx->status = MCF_OPTIMAL;
            HIP_TRY(h, hipMemcpyAsync(&h->d_ctx->status, &h->h_ctx->status, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
    }
    if (h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "internal error: preorder permutation did not close"; return MCF_E_INTERNAL; }
    h->stats.solve_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    h->solved_once = true;
    return MCF_OK;
}

// Independent instances side by side: one launch per engine path, one persistent workgroup per handle
// (k_solve_small_batch: whole instance in LDS; k_solve_mid_batch: state in global memory, Dantzig / Devex).
int mcf_solve_batch(mcf_handle* const* handles, int32_t count, const int64_t* max_pivots, double* kernel_ms) {
    if (!handles || count <= 0) return MCF_E_BAD_ARG;
    mcf_handle* h0 = handles[0];
    if (!h0) return MCF_E_BAD_ARG;
    for (int32_t i = 0; i < count; ++i) {
        mcf_handle* h = handles[i];
        if (!h) return MCF_E_BAD_ARG;
        const bool loop = h->small || h->mid;
        if (!loop || h->shards != 1 || h->device != h0->device) {
            h0->err = "mcf_solve_batch: every handle must run as ONE persistent workgroup -- mcf_stats.pricing_mode 2 (LDS loop) or 3 "
                      "(persistent loop; mcf_options.mid_loop = 1 asks for it at any size) -- on one device";
            return MCF_E_STATE;
        }
        for (int32_t j = 0; j < i; ++j)
            if (handles[j] == h) { h0->err = "mcf_solve_batch: a handle appears twice"; return MCF_E_BAD_ARG; }
    }
    HIP_TRY(h0, hipSetDevice(h0->device));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<SmallJob> small_jobs;
    std::vector<MidJob> mid_jobs;
    uint32_t lds = 0;
    const bool batch_narrow_ok = small_narrow_allowed();
    for (int32_t i = 0; i < count; ++i) {
        mcf_handle* h = handles[i];
        int rc = sync_ctx(h, h->stream);   // (also drains whatever the handle's own stream still holds)
        if (rc) return rc;
        h->external_driver = false;
        const int64_t m = h->im.m, n = h->im.n;
        int64_t mp = max_pivots ? max_pivots[i] : -1;
        if (mp < 0) mp = 20 * (m + n) > 100 ? 20 * (m + n) : 100;  // simplex.py:1470
        const int64_t cap = h->h_ctx->pivots + mp;
        if (h->small) {
            SmallJob J;
            J.g = h->view; J.L = h->small_layout; J.rule = h->opt.rule; J.narrow = small_narrow_for(h->im, batch_narrow_ok);
            J.list = h->d_cand; J.cap = cap; J.host_ctx = h->h_ctx;
            h->stats.small_narrow = J.narrow;
            small_jobs.push_back(J);
            if (h->small_layout.total > lds) lds = h->small_layout.total;
        } else {
            MidJob J;
            J.g = h->view; J.rule = h->opt.rule; J.nlist = h->price_blocks; J.list = h->d_cand; J.cap = cap; J.host_ctx = h->h_ctx;
            mid_jobs.push_back(J);
        }
    }
    // candidate-list jobs last (their own launch)
    std::stable_partition(mid_jobs.begin(), mid_jobs.end(), [](const MidJob& J) { return J.rule != MCF_RULE_CANDIDATE_LIST; });
    // ... and the LDS jobs of the front kernel behind the others (small_front_for: a launch each)
    auto job_front = [](const SmallJob& J) { return small_front_for(J.narrow, J.rule, J.g.key_mode, J.g); };
    std::stable_partition(small_jobs.begin(), small_jobs.end(), [&](const SmallJob& J) { return !job_front(J); });
    size_t n_front = 0;
    for (const SmallJob& J : small_jobs) n_front += job_front(J) ? 1 : 0;
    size_t n_listing = 0;
    for (const MidJob& J : mid_jobs) n_listing += J.rule == MCF_RULE_CANDIDATE_LIST ? 1 : 0;
    // job arrays and the two timing events come from a per-device pool that only ever grows (a call used to pay two
    // hipMalloc / hipFree pairs and two event creations); the pool's lock also serialises concurrent batches on a device
    struct BatchPool { void* small = nullptr; size_t small_bytes = 0; void* mid = nullptr; size_t mid_bytes = 0; hipEvent_t ev[2] = {nullptr, nullptr}; };
    static std::mutex pool_mu;
    static BatchPool pools[64];
    std::lock_guard<std::mutex> pool_lock(pool_mu);
    BatchPool& pool = pools[h0->device & 63];
    SmallJob* d_small = nullptr;
    MidJob* d_mid = nullptr;
    auto cleanup = [&]() {};   // (nothing is owned by the call any more)
    auto bail = [&](const char* what, hipError_t e) {
        h0->err = std::string(what) + ": " + hipGetErrorString(e);
        cleanup();
        return MCF_E_HIP;
    };
    hipError_t e;
    hipStream_t s = h0->stream;
    auto grow = [&](void** buf, size_t* have, size_t need) -> hipError_t {
        if (need <= *have) return hipSuccess;
        if (*buf) (void)hipFree(*buf);
        *buf = nullptr; *have = 0;
        const hipError_t ge = hipMalloc(buf, need * 2);
        if (ge == hipSuccess) *have = need * 2;
        return ge;
    };
    if (!small_jobs.empty()) {
        if ((e = grow(&pool.small, &pool.small_bytes, small_jobs.size() * sizeof(SmallJob))) != hipSuccess) return bail("hipMalloc jobs", e);
        d_small = static_cast<SmallJob*>(pool.small);
        if ((e = hipMemcpyAsync(d_small, small_jobs.data(), small_jobs.size() * sizeof(SmallJob), hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpy jobs", e);
    }
    if (!mid_jobs.empty()) {
        if ((e = grow(&pool.mid, &pool.mid_bytes, mid_jobs.size() * sizeof(MidJob))) != hipSuccess) return bail("hipMalloc jobs", e);
        d_mid = static_cast<MidJob*>(pool.mid);
        if ((e = hipMemcpyAsync(d_mid, mid_jobs.data(), mid_jobs.size() * sizeof(MidJob), hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpy jobs", e);
    }
    if (!pool.ev[0] && ((e = hipEventCreate(&pool.ev[0])) != hipSuccess || (e = hipEventCreate(&pool.ev[1])) != hipSuccess)) return bail("hipEventCreate", e);
    hipEvent_t* ev = pool.ev;
    if ((e = hipEventRecord(ev[0], s)) != hipSuccess) return bail("hipEventRecord", e);
    if (!small_jobs.empty()) {
        // Any handle runs at either width: the width belongs to the launch.  A batch runs at 256 lanes like a single solve
        // (scripts/batch_small.py per width, DESIGN.md: 43.7 M pivots/s over 1 024 instances against 33.1 M at 1 024 lanes)
        // unless MCF_SMALL_THREADS forces 1 024.
        const bool w1024 = small_threads_forced() == 1024;
        const unsigned n_rest = (unsigned)(small_jobs.size() - n_front);
        const SmallJob* rest = d_small;
        const SmallJob* fronts = d_small + n_rest;
        const int width = w1024 ? 1024 : 256;
        if (n_rest) hipLaunchKernelGGL(small_batch_kernel(width, false), dim3(n_rest), dim3(width), lds, s, rest);
        if (n_front) hipLaunchKernelGGL(small_batch_kernel(width, true), dim3((unsigned)n_front), dim3(width), lds, s, fronts);
    }
    {
        // Two narrow workgroups per CU pay when there are more instances than CUs and the per-pivot passes are short
        // (measured, 512 instances: 1 024 nodes 1.4x, 4 096 nodes 1.06x; with <= 256 instances a narrow workgroup only has
        // half the lanes: 0.75-0.9x).  MCF_BATCH_THREADS = 512 / 1024 forces either.
        const char* bt = std::getenv("MCF_BATCH_THREADS");
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h0->device);
        int32_t max_nodes = 0;
        for (const MidJob& J : mid_jobs) if (J.g.n_nodes > max_nodes) max_nodes = J.g.n_nodes;
        const bool wide = bt ? std::atoi(bt) == 1024 : !((int)mid_jobs.size() > cus && max_nodes <= 4096);
        // the candidate-list jobs sit behind the others in the array (sorted above) and get the kernel that sweeps for itself
        const unsigned n_plain = (unsigned)(mid_jobs.size() - n_listing), n_list = (unsigned)n_listing;
        const MidJob* plain = d_mid;
        const MidJob* lists = d_mid ? d_mid + n_plain : nullptr;
        if (n_plain && wide) hipLaunchKernelGGL((k_solve_mid_batch<1024, false>), dim3(n_plain), dim3(1024), 0, s, plain);
        else if (n_plain) hipLaunchKernelGGL((k_solve_mid_batch<512, false>), dim3(n_plain), dim3(512), 0, s, plain);
        if (n_list && wide) hipLaunchKernelGGL((k_solve_mid_batch<1024, true>), dim3(n_list), dim3(1024), 0, s, lists);
        else if (n_list) hipLaunchKernelGGL((k_solve_mid_batch<512, true>), dim3(n_list), dim3(512), 0, s, lists);
    }
    if ((e = hipGetLastError()) != hipSuccess) return bail("mcf_solve_batch launch", e);
    // (every workgroup writes its final control block straight into its handle's pinned host copy: nothing to read back)
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail("hipStreamSynchronize", e);
    // A persistent-loop launch runs at most 2^22 loop iterations per job: a job that is still RUNNING below its budget
    // (large mid_loop = 1 instances) goes round again, like mcf_solve's loop, instead of coming back as "iteration limit".
    for (int round = 0; round < 4096 && !mid_jobs.empty(); ++round) {
        std::vector<MidJob> again_plain, again_list;
        for (const MidJob& J : mid_jobs) {
            const McfCtx* hc = J.host_ctx;
            if (hc->status == MCF_RUNNING && hc->pivots < J.cap) (J.rule == MCF_RULE_CANDIDATE_LIST ? again_list : again_plain).push_back(J);
        }
        if (again_plain.empty() && again_list.empty()) break;
        std::vector<MidJob> again(again_plain);
        again.insert(again.end(), again_list.begin(), again_list.end());
        if ((e = hipMemcpyAsync(d_mid, again.data(), again.size() * sizeof(MidJob), hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpy jobs", e);
        if (!again_plain.empty()) hipLaunchKernelGGL((k_solve_mid_batch<1024, false>), dim3((unsigned)again_plain.size()), dim3(1024), 0, s, (const MidJob*)d_mid);
        if (!again_list.empty()) hipLaunchKernelGGL((k_solve_mid_batch<1024, true>), dim3((unsigned)again_list.size()), dim3(1024), 0, s, (const MidJob*)(d_mid + again_plain.size()));
        if ((e = hipGetLastError()) != hipSuccess) return bail("mcf_solve_batch relaunch", e);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail("hipStreamSynchronize", e);
    }
    if ((e = hipEventRecord(ev[1], s)) != hipSuccess) return bail("hipEventRecord", e);
    if ((e = hipEventSynchronize(ev[1])) != hipSuccess) return bail("hipEventSynchronize", e);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (kernel_ms) *kernel_ms = ms;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    int ret = MCF_OK;
    for (int32_t i = 0; i < count; ++i) {
        mcf_handle* h = handles[i];
        h->ctx_current = true;
        h->stats.batches += 1;
        h->stats.solve_seconds += secs / count;   // the batch's wall time, shared out
        h->solved_once = true;
        if (h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "internal error: preorder permutation did not close"; ret = MCF_E_INTERNAL; }
    }
    cleanup();
    return ret;
}

int mcf_get_result(mcf_handle* h, int32_t* status, int64_t* objective_hi_lo, int64_t* flow, int64_t* potential,
                   int8_t* in_tree, mcf_stats* stats) {
    if (!h) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = sync_ctx(h, h->stream);
    if (rc) return rc;
    const McfHostImage& im = h->im;
    // the flow copy (16 B per arc) is only made when something derived from it is asked for
    const bool need_arcw = status || objective_hi_lo || flow;
    std::vector<McfArcW> arcw;
    McfHostResult r;
    r.artificial_flow = -1;
    if (need_arcw) {
        arcw.resize(im.arcw.size());
        HIP_TRY(h, hipMemcpy(arcw.data(), h->d_arcw, arcw.size() * sizeof(McfArcW), hipMemcpyDeviceToHost));
        mcf_extract(im, arcw, h->h_ctx->status, r);
    }
    if (status) *status = r.status;
    if (objective_hi_lo) {
        objective_hi_lo[0] = (int64_t)(r.objective >> 64);
        objective_hi_lo[1] = (int64_t)(uint64_t)r.objective;
    }
    if (flow) for (int64_t i = 0; i < im.m; ++i) flow[im.orig[i]] = arcw[i].flow;  // engine order -> caller's
    if (potential) {
        std::vector<int64_t> pi(im.n_nodes);
        HIP_TRY(h, hipMemcpy(pi.data(), h->d_pi, pi.size() * 8, hipMemcpyDeviceToHost));
        for (int32_t v = 0; v < im.n; ++v) potential[v] = pi[v] - pi[im.n];
    }
    if (in_tree) {
        std::vector<int8_t> st(im.m_pad);
        HIP_TRY(h, hipMemcpy(st.data(), h->d_state, st.size(), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < im.m; ++i) in_tree[im.orig[i]] = st[i] == 0;
    }
    if (stats) {
        const McfCtx& c = *h->h_ctx;
        h->stats.pivots = c.pivots; h->stats.degenerate = c.degenerate; h->stats.bound_flips = c.bound_flips;
        h->stats.arcs_priced = c.arcs_priced; h->stats.nodes_moved = c.nodes_moved;
        h->stats.subtree_nodes = c.subtree_nodes; h->stats.cycle_arcs = c.cycle_arcs;
        h->stats.unbounded_arc = c.unbounded_arc >= 0 ? im.orig[c.unbounded_arc] : -1;
        h->stats.artificial_flow = r.artificial_flow;
        h->stats.pricing_mode = h->small ? 2 : (h->mid ? 3 : (h->rcached ? 1 : 0));
        h->stats.sweep_variant = ((h->view.vkey && h->opt.rule != MCF_RULE_DEVEX_BLOCK) ? 1 : 0) | (h->view.vkey && h->nt_sweep ? 2 : 0) | (h->view.dirty ? 4 : 0);
        h->stats.tree_blocks = h->bpl ? h->bpl_shift : 0; h->stats.tree_rebuilds = c.rebuilds;
        h->stats.run_pairs = h->run_pairs;
        h->stats.cycle_scans = c.scans; h->stats.scan_rounds = c.scan_rounds; {
            h->stats.arcs_swept = c.arcs_priced;  // full sweeps read what they cover ...
            if (h->view.dirty) {                   // ... incremental ones count per pricing workgroup
                std::vector<int64_t> sw(kMaxPriceBlocks);
                HIP_TRY(h, hipMemcpy(sw.data(), h->d_swept, sw.size() * 8, hipMemcpyDeviceToHost));
                h->stats.arcs_swept = 0;
                for (int64_t x : sw) h->stats.arcs_swept += x;
            }
        }
        h->stats.unbounded_rc = 0;
        if (c.status == MCF_UNBOUNDED && c.unbounded_arc >= 0) {
            std::vector<int64_t> pi(im.n_nodes);
            HIP_TRY(h, hipMemcpy(pi.data(), h->d_pi, pi.size() * 8, hipMemcpyDeviceToHost));
            const int64_t a = c.unbounded_arc;
            const int64_t rcost = im.cost64[a] + pi[im.tail[a]] - pi[im.head[a]];
            h->stats.unbounded_rc = rcost < 0 ? rcost : -rcost;
        }
        *stats = h->stats;
    }
    return MCF_OK;
}

int mcf_price_once(mcf_handle* h, int32_t rule, int64_t start, int64_t end, int64_t* arc, int32_t* dir, int64_t* key) {
    if (!h || !arc) return MCF_E_BAD_ARG;
    if (rule == MCF_RULE_CANDIDATE_LIST) rule = MCF_RULE_DANTZIG_FULL;  // the list is built by a Dantzig sweep
    if (rule != MCF_RULE_DANTZIG_FULL && rule != MCF_RULE_DEVEX_BLOCK) return MCF_E_BAD_ARG;
    if (start < 0 || end > h->im.m || start > end) { h->err = "mcf_price_once: bad range"; return MCF_E_BAD_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    // price even when the solve has finished: temporarily view the control block as running
    McfView v = h->view;
    v.dirty = nullptr;  // a parity hook prices everything and leaves the flags alone
    v.candx = nullptr;  // ... and the live list's records
    if (rule == MCF_RULE_DEVEX_BLOCK) v.weight = h->d_weight;
    HIP_TRY(h, hipMemcpyAsync(h->h_ctx, h->d_ctx, sizeof(McfCtx), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int32_t saved = h->h_ctx->status;
    int32_t running = MCF_RUNNING;
    HIP_TRY(h, hipMemcpyAsync(&h->d_ctx->status, &running, 4, hipMemcpyHostToDevice, h->stream));
    // whole arc list (shard 0 of 1), restricted to ORIGINAL indices [start, end)
    {
        const dim3 grid(h->price_blocks), block(kPriceThreads);
        const int64_t z = 0, one = 1;
        if (h->rcached) {
            if (rule == MCF_RULE_DEVEX_BLOCK)
                hipLaunchKernelGGL((k_price_rc<MCF_RULE_DEVEX_BLOCK, true, false>), grid, block, 0, h->stream, v, z, one, 0, start, end, h->d_cand_aux, (int64_t*)nullptr, (const int32_t*)nullptr);
            else
                hipLaunchKernelGGL((k_price_rc<MCF_RULE_DANTZIG, true, false>), grid, block, 0, h->stream, v, z, one, 0, start, end, h->d_cand_aux, (int64_t*)nullptr, (const int32_t*)nullptr);
        } else {
            if (rule == MCF_RULE_DEVEX_BLOCK)
                hipLaunchKernelGGL((k_price<MCF_RULE_DEVEX_BLOCK, true>), grid, block, 0, h->stream, v, z, one, 0, start, end, h->d_cand_aux);
            else
                hipLaunchKernelGGL((k_price<MCF_RULE_DANTZIG, true>), grid, block, 0, h->stream, v, z, one, 0, start, end, h->d_cand_aux);
        }
    }
    hipLaunchKernelGGL(k_reduce, dim3(1), dim3(kReduceThreads), 0, h->stream, h->d_cand_aux, h->price_blocks, h->d_one);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(&h->d_ctx->status, &saved, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->h_one, h->d_one, sizeof(McfCand), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const bool found = h->h_one->key > 0 && h->h_one->arc >= 0;
    *arc = found ? ((h->h_one->arc >> 32) & (MCF_DIR_FLAG - 1)) : -1;  // caller's arc index (Devex ids carry the direction in bit 30)
    // Devex and the capacity-weighted variant report their merit (bit pattern of the double), the other variants the violation
    if (key) *key = found ? ((rule == MCF_RULE_DEVEX_BLOCK || h->view.key_mode == MCF_KEY_CAPACITY) ? h->h_one->key : (h->h_one->key & ~MCF_FWD_BIT)) : 0;
    if (dir) {
        *dir = 0;
        if (found) {
            int8_t st = 0;
            HIP_TRY(h, hipMemcpy(&st, h->d_state + (h->h_one->arc & 0xffffffff), 1, hipMemcpyDeviceToHost));
            *dir = st;
        }
    }
    return MCF_OK;
}

int mcf_enqueue_price(mcf_handle* h, void* stream, int64_t* cand_out_dev) {
    if (!h || !cand_out_dev) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int32_t rule = h->opt.rule;
    h->ctx_current = false;
    h->external_driver = true;
    launch_price(h, s, h->view, rule, rule != MCF_RULE_DANTZIG);
    hipLaunchKernelGGL(k_reduce, dim3(1), dim3(kReduceThreads), 0, s, h->d_cand, h->price_blocks,
                       reinterpret_cast<McfCand*>(cand_out_dev));
    HIP_TRY(h, hipGetLastError());
    return MCF_OK;
}

int mcf_enqueue_pivot(mcf_handle* h, void* stream, const int64_t* cands_dev, int32_t ncand) {
    if (!h || !cands_dev || ncand < 1) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    h->ctx_current = false;
    h->external_driver = true;
    launch_k_pivot(h, s, reinterpret_cast<const McfCand*>(cands_dev), ncand, h->opt.rule, 1);
    launch_apply(h, s);
    HIP_TRY(h, hipGetLastError());
    return MCF_OK;
}

int mcf_shard_info(mcf_handle* h, int32_t* list_len, int32_t* minor_cap) {
    if (!h) return MCF_E_BAD_ARG;
    if (list_len) *list_len = h->price_blocks;
    if (minor_cap) *minor_cap = mcf_minor_cap(h->price_blocks);
    return MCF_OK;
}

int mcf_enqueue_price_list(mcf_handle* h, void* stream, int64_t* cands_out_dev) {
    if (!h || !cands_out_dev) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int32_t rule = h->opt.rule;
    h->ctx_current = false;
    h->external_driver = true;
    // the pricing grid writes one candidate per workgroup straight into the caller's buffer (price_blocks entries);
    // candidate-list rule: a no-op while minor iterations are pending, so the buffer keeps the live list
    launch_price(h, s, h->view, rule, rule != MCF_RULE_DANTZIG, reinterpret_cast<McfCand*>(cands_out_dev));
    HIP_TRY(h, hipGetLastError());
    return MCF_OK;
}

int mcf_enqueue_pivots(mcf_handle* h, void* stream, const int64_t* cands_dev, int32_t ncand, int32_t count) {
    if (!h || !cands_dev || ncand < 1 || count < 1) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    h->ctx_current = false;
    h->external_driver = true;
    for (int i = 0; i < count; ++i) {  // slot 0 takes the fresh list, the others re-price it (minor iterations)
        launch_k_pivot(h, s, reinterpret_cast<const McfCand*>(cands_dev), ncand, h->opt.rule, i == 0 ? 1 : 0);
        launch_apply(h, s);
    }
    HIP_TRY(h, hipGetLastError());
    return MCF_OK;
}

int mcf_poll(mcf_handle* h, void* stream, int32_t* status_or_running, int64_t* pivots) {
    if (!h) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = sync_ctx(h, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    if (h->h_ctx->status == MCF_INTERNAL_ERROR) { h->err = "internal error: preorder permutation did not close"; return MCF_E_INTERNAL; }
    if (status_or_running) {
        const int32_t st = h->h_ctx->status;
        // infeasibility (artificial flow left) is only resolved by mcf_get_result
        *status_or_running = st == MCF_RUNNING ? -1 : st == MCF_OPTIMAL ? MCF_ST_OPTIMAL
                             : st == MCF_UNBOUNDED ? MCF_ST_UNBOUNDED : MCF_ST_ITERATION_LIMIT;
    }
    if (pivots) *pivots = h->h_ctx->pivots;
    return MCF_OK;
}

int mcf_time_pricing(mcf_handle* h, int32_t rule, int32_t reps, double* ms_per_launch) {
    if (!h || !ms_per_launch || reps < 1) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    McfView v = h->view;
    v.dirty = nullptr;  // timed sweeps are full sweeps
    v.candx = nullptr;  // (and leave the live list's records alone)
    if (rule == MCF_RULE_DEVEX_BLOCK) v.weight = h->d_weight;
    HIP_TRY(h, hipMemcpyAsync(h->h_ctx, h->d_ctx, sizeof(McfCtx), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int32_t saved = h->h_ctx->status;
    int32_t running = MCF_RUNNING;
    HIP_TRY(h, hipMemcpyAsync(&h->d_ctx->status, &running, 4, hipMemcpyHostToDevice, h->stream));
    hipEvent_t e0, e1;
    HIP_TRY(h, hipEventCreate(&e0));
    HIP_TRY(h, hipEventCreate(&e1));
    auto once = [&]() { launch_price(h, h->stream, v, rule == MCF_RULE_CANDIDATE_LIST ? MCF_RULE_DANTZIG : rule, rule == MCF_RULE_DEVEX_BLOCK, h->d_cand_aux); };
    once();  // warm
    HIP_TRY(h, hipEventRecord(e0, h->stream));
    for (int i = 0; i < reps; ++i) once();
    HIP_TRY(h, hipEventRecord(e1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&h->d_ctx->status, &saved, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = (double)ms / reps;
    return MCF_OK;
}

int mcf_time_copy(int32_t device, int64_t bytes, int32_t reps, double* ms_per_copy) {
    if (!ms_per_copy || bytes < 16 || reps < 1) return MCF_E_BAD_ARG;
    if (usable_devices() <= 0) return MCF_E_NO_DEVICE;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return MCF_E_HIP;
    uint4 *a = nullptr, *b = nullptr;
    const int64_t n16 = bytes / 16;
    if (hipMalloc(reinterpret_cast<void**>(&a), n16 * 16) != hipSuccess) return MCF_E_ALLOC;
    if (hipMalloc(reinterpret_cast<void**>(&b), n16 * 16) != hipSuccess) { (void)hipFree(a); return MCF_E_ALLOC; }
    (void)hipMemset(a, 1, n16 * 16);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(k_copy16, dim3(2048), dim3(256), 0, nullptr, a, b, n16);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_copy16, dim3(2048), dim3(256), 0, nullptr, a, b, n16);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    *ms_per_copy = (double)ms / reps;
    return hipGetLastError() == hipSuccess ? MCF_OK : MCF_E_HIP;
}

int mcf_get_tree(mcf_handle* h, int32_t* parent, int32_t* pred_arc, int32_t* size, int32_t* pos, int32_t* order,
                 int8_t* state, int64_t* potential_with_root, int32_t* depth, int32_t* psize) {
    if (!h) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = read_ctx(h, h->stream);
    if (rc) return rc;
    const McfHostImage& im = h->im;
    std::vector<McfNode> nodes(im.n_nodes);
    HIP_TRY(h, hipMemcpy(nodes.data(), h->d_node, nodes.size() * sizeof(McfNode), hipMemcpyDeviceToHost));
    for (int32_t v = 0; v < im.n_nodes; ++v) {
        if (parent) parent[v] = nodes[v].parent;
        if (pred_arc) {
            const int64_t a = nodes[v].pred < 0 ? -1 : nodes[v].pred >> 1;
            pred_arc[v] = a < 0 ? -1 : (a < im.m ? im.orig[a] : (int32_t)a);  // artificial arcs keep m + node
        }
        if (size) size[v] = nodes[v].size;
        if (depth) depth[v] = nodes[v].depth;
    }
    const int cur = tree_sel(*h->h_ctx).cur, arena = tree_sel(*h->h_ctx).arena;
    if (h->bpl) {
        // blocked preorder list: flatten the blocks handed out so far into the logical arrays the dense layout would hold
        const int32_t nb = h->h_ctx->alloc_next;
        const size_t slots = (size_t)nb << h->bpl_shift;
        std::vector<int32_t> tok(slots), psz(slots), ext((size_t)nb);
        std::vector<McfBlkMeta> meta((size_t)nb);
        HIP_TRY(h, hipMemcpy(tok.data(), arena ? h->d_order1 : h->d_order0, slots * 4, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(psz.data(), arena ? h->d_psz1 : h->d_psz0, slots * 4, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(meta.data(), h->d_bmeta[cur], (size_t)nb * sizeof(McfBlkMeta), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(ext.data(), h->d_bext[arena], (size_t)nb * 4, hipMemcpyDeviceToHost));
        std::vector<int32_t> ford((size_t)im.n_nodes, -1), fpos((size_t)im.n_nodes, -1), fpsz((size_t)im.n_nodes, -1);
        if (!mcf_bpl_flatten(im.n_nodes, h->bpl_shift, nb, tok.data(), psz.data(), meta.data(), ext.data(), ford.data(), fpos.data(), fpsz.data())) {
            h->err = "internal error: the blocked preorder list does not tile the positions";
            return MCF_E_INTERNAL;
        }
        for (int32_t v = 0; v < im.n_nodes; ++v) {
            if (order) order[v] = ford[v];
            if (pos) pos[v] = fpos[v];
            if (psize) psize[v] = fpsz[v];
        }
        order = nullptr; pos = nullptr; psize = nullptr;
    }
    if (order) HIP_TRY(h, hipMemcpy(order, cur ? h->d_order1 : h->d_order0, (size_t)im.n_nodes * 4, hipMemcpyDeviceToHost));
    if (pos) HIP_TRY(h, hipMemcpy(pos, cur ? h->d_pos1 : h->d_pos0, (size_t)im.n_nodes * 4, hipMemcpyDeviceToHost));
    if (psize) {
        if (h->d_psz0) HIP_TRY(h, hipMemcpy(psize, cur ? h->d_psz1 : h->d_psz0, (size_t)im.n_nodes * 4, hipMemcpyDeviceToHost));
        else for (int32_t v = 0; v < im.n_nodes; ++v) psize[v] = -1;  // not kept for this handle
    }
    if (state) {
        std::vector<int8_t> st(im.m_pad);
        HIP_TRY(h, hipMemcpy(st.data(), h->d_state, st.size(), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < im.m; ++i) state[im.orig[i]] = st[i];
    }
    if (potential_with_root) HIP_TRY(h, hipMemcpy(potential_with_root, h->d_pi, (size_t)im.n_nodes * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

int mcf_get_reduced_costs(mcf_handle* h, int64_t* rc_out, int32_t* resident) {
    if (!h || !rc_out) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const McfHostImage& im = h->im;
    if (resident) *resident = h->rcached ? 1 : 0;
    if (h->rcached) {
        std::vector<int64_t> rc(im.m_pad);
        HIP_TRY(h, hipMemcpy(rc.data(), h->d_rcache, rc.size() * 8, hipMemcpyDeviceToHost));
        if (h->view.rc_partial) {  // a sharded handle keeps only its own shard exact: the other arcs from the potentials
            std::vector<int64_t> pi(im.n_nodes);
            HIP_TRY(h, hipMemcpy(pi.data(), h->d_pi, pi.size() * 8, hipMemcpyDeviceToHost));
            std::vector<int8_t> mine(im.m, 0);
            for (int x = 0; x < MCF_NUM_BUCKETS; ++x) {
                int64_t lo, hi;
                mcf_bucket_slice(im.bucket_off, x, h->shard, h->shards, 0, 1, &lo, &hi);
                for (int64_t e2 = lo; e2 < hi; ++e2) mine[e2] = 1;
            }
            for (int64_t i = 0; i < im.m; ++i) if (!mine[i]) rc[i] = im.cost64[i] + pi[im.tail[i]] - pi[im.head[i]];
            if (resident) *resident = 2;  // own shard resident
        }
        for (int64_t i = 0; i < im.m; ++i) rc_out[im.orig[i]] = rc[i];
    } else {
        std::vector<int64_t> pi(im.n_nodes);
        HIP_TRY(h, hipMemcpy(pi.data(), h->d_pi, pi.size() * 8, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < im.m; ++i) rc_out[im.orig[i]] = im.cost64[i] + pi[im.tail[i]] - pi[im.head[i]];
    }
    return MCF_OK;
}

int mcf_get_pricing_keys(mcf_handle* h, int32_t* keys_out, int32_t* present) {
    if (!h || !keys_out) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const McfHostImage& im = h->im;
    if (present) *present = h->d_vkey ? 1 : 0;
    if (!h->d_vkey) { for (int64_t i = 0; i < im.m; ++i) keys_out[i] = 0; return MCF_OK; }
    std::vector<int32_t> vk(im.m_pad);
    HIP_TRY(h, hipMemcpy(vk.data(), h->d_vkey, vk.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < im.m; ++i) keys_out[im.orig[i]] = vk[i];
    return MCF_OK;
}

int mcf_get_weights(mcf_handle* h, float* weight_out) {
    if (!h || !weight_out) return MCF_E_BAD_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const McfHostImage& im = h->im;
    std::vector<float> w(im.m_pad);
    HIP_TRY(h, hipMemcpy(w.data(), h->d_weight, w.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < im.m; ++i) weight_out[im.orig[i]] = w[i];
    return MCF_OK;
}

#ifdef MCF_STAMPS
int mcf_debug_stamps(mcf_handle* h, unsigned long long* out8) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out8, h->d_rec1, 64, hipMemcpyDeviceToHost));
    return MCF_OK;
}
#ifdef MCF_WAVE_STAMPS
// the fused LDS loop's per-wave clocks: six words per wave, 16 waves (MCF_WAVE_STAMP)
int mcf_debug_wave_stamps(mcf_handle* h, unsigned long long* out96) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::memset(out96, 0, 16 * 6 * 8);
    if ((int64_t)h->im.n_nodes * (int64_t)sizeof(McfNode) < (8 + 16 * 6) * 8) return MCF_OK;   // (the kernel wrote none: its guard)
    HIP_TRY(h, hipMemcpy(out96, reinterpret_cast<const char*>(h->d_rec1) + 64, 16 * 6 * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
#endif
// k_pivot phase stamps (24 slots, [23] = launches that pivoted); clear = 1 zeroes them afterwards
int mcf_debug_pivot_stamps(mcf_handle* h, unsigned long long* out24, int clear) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_pivot_stamps), 24 * 8));
    if (clear) { unsigned long long z[24] = {0}; HIP_TRY(h, hipMemcpyToSymbol(HIP_SYMBOL(g_pivot_stamps), z, 24 * 8)); }
    return MCF_OK;
}
#endif

// ---------------------------------------------------------------------------------------------
// native DIMACS reader (host code; benchmarks/parsers/dimacs.py:105-286 restated for flat arrays)
// ---------------------------------------------------------------------------------------------
extern "C++" {
namespace {
int dimacs_fail(char* err, int32_t err_len, const std::string& msg) {
    if (err && err_len > 0) { std::snprintf(err, (size_t)err_len, "%s", msg.c_str()); }
    return MCF_E_BAD_ARG;
}

// parse one integer token; "inf" and values >= 1e15 map to `inf_value` when allow_inf
bool dimacs_int(const char*& p, int64_t* out, bool allow_inf, int64_t inf_value) {
    while (*p == ' ' || *p == '\t') ++p;
    if (allow_inf && (p[0] == 'i' || p[0] == 'I') && (p[1] == 'n' || p[1] == 'N') && (p[2] == 'f' || p[2] == 'F')) {
        p += 3;
        *out = inf_value;
        return true;
    }
    char* end = nullptr;
    errno = 0;
    const long long v = std::strtoll(p, &end, 10);
    if (end == p || errno) return false;
    if (*end == '.' || *end == 'e' || *end == 'E') {  // "12.0" is fine, "12.5" is not integral
        char* fend = nullptr;
        const double d = std::strtod(p, &fend);
        if (fend == p || d != (double)(long long)d) return false;
        p = fend;
        *out = allow_inf && d >= 1e15 ? inf_value : (int64_t)d;
        return true;
    }
    p = end;
    *out = allow_inf && v >= 1000000000000000LL ? inf_value : (int64_t)v;
    return true;
}

template <typename OnProblem, typename OnNode, typename OnArc>
int dimacs_walk(const char* path, char* err, int32_t err_len, OnProblem on_p, OnNode on_n, OnArc on_a) {
    FILE* f = std::fopen(path, "r");
    if (!f) return dimacs_fail(err, err_len, std::string("DIMACS file not found: ") + path);
    std::vector<char> line(1 << 16);
    int64_t line_no = 0;
    bool seen_p = false;
    int rc = 0;
    while (rc == 0 && std::fgets(line.data(), (int)line.size(), f)) {
        ++line_no;
        const char* p = line.data();
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == 0 || *p == '\n' || *p == '\r' || *p == 'c') continue;
        const char kind = *p++;
        const std::string where = "Line " + std::to_string(line_no) + ": ";
        if (kind == 'p') {
            if (seen_p) { rc = dimacs_fail(err, err_len, where + "Multiple problem descriptor lines found."); break; }
            while (*p == ' ' || *p == '\t') ++p;
            if (std::strncmp(p, "min", 3) != 0) { rc = dimacs_fail(err, err_len, where + "Only 'min' (minimum cost flow) problems supported."); break; }
            p += 3;
            int64_t n = 0, m = 0;
            if (!dimacs_int(p, &n, false, 0) || !dimacs_int(p, &m, false, 0)) { rc = dimacs_fail(err, err_len, where + "Expected 'p min <nodes> <arcs>'."); break; }
            if (n <= 0) { rc = dimacs_fail(err, err_len, where + "Number of nodes must be positive."); break; }
            if (m < 0) { rc = dimacs_fail(err, err_len, where + "Number of arcs cannot be negative."); break; }
            seen_p = true;
            rc = on_p(n, m, where);
        } else if (kind == 'n') {
            if (!seen_p) { rc = dimacs_fail(err, err_len, where + "Node descriptor before problem descriptor."); break; }
            int64_t id = 0, sup = 0;
            if (!dimacs_int(p, &id, false, 0) || !dimacs_int(p, &sup, false, 0)) { rc = dimacs_fail(err, err_len, where + "Expected 'n <node_id> <supply>' with integer data."); break; }
            rc = on_n(id, sup, where);
        } else if (kind == 'a') {
            if (!seen_p) { rc = dimacs_fail(err, err_len, where + "Arc descriptor before problem descriptor."); break; }
            int64_t v[5];
            int k = 0;
            // tail head [lower] cap cost : the capacity token is the second-to-last one
            const char* q = p;
            int tokens = 0;
            for (const char* t = p; *t;) {
                while (*t == ' ' || *t == '\t') ++t;
                if (*t == 0 || *t == '\n' || *t == '\r') break;
                ++tokens;
                while (*t && *t != ' ' && *t != '\t' && *t != '\n' && *t != '\r') ++t;
            }
            if (tokens != 4 && tokens != 5) { rc = dimacs_fail(err, err_len, where + "Invalid arc descriptor format."); break; }
            bool ok = true;
            for (k = 0; k < tokens && ok; ++k) ok = dimacs_int(q, &v[k], k == tokens - 2, -1);
            if (!ok) { rc = dimacs_fail(err, err_len, where + "Failed to parse arc line (integer data expected)."); break; }
            const int64_t lower = tokens == 5 ? v[2] : 0;
            int64_t cap = v[tokens - 2];
            if (cap < 0) cap = -1;
            rc = on_a(v[0], v[1], lower, cap, v[tokens - 1], where);
        } else {
            rc = dimacs_fail(err, err_len, where + "Unknown line type '" + std::string(1, kind) + "'.");
        }
    }
    std::fclose(f);
    if (rc == 0 && !seen_p) rc = dimacs_fail(err, err_len, "No problem descriptor found. DIMACS file must contain a 'p min <nodes> <arcs>' line.");
    return rc;
}
}  // namespace
}  // extern "C++"

int mcf_dimacs_scan(const char* path, int64_t* n_nodes, int64_t* n_arcs, char* err, int32_t err_len) {
    if (!path || !n_nodes || !n_arcs) return MCF_E_BAD_ARG;
    int64_t n = 0, m = 0, arcs = 0;
    const int rc = dimacs_walk(
        path, err, err_len, [&](int64_t nn, int64_t mm, const std::string&) { n = nn; m = mm; return 0; },
        [&](int64_t, int64_t, const std::string&) { return 0; },
        [&](int64_t, int64_t, int64_t, int64_t, int64_t, const std::string&) { ++arcs; return 0; });
    if (rc) return rc;
    if (arcs != m)
        return dimacs_fail(err, err_len, "Arc count mismatch: problem descriptor specifies " + std::to_string(m) + " arcs, but " +
                                             std::to_string(arcs) + " arc descriptors found.");
    *n_nodes = n;
    *n_arcs = m;
    return MCF_OK;
}

int mcf_dimacs_load(const char* path, int64_t n_nodes, int64_t n_arcs, int32_t* tail, int32_t* head, int64_t* lower,
                    int64_t* cap, int64_t* cost, int64_t* supply, char* err, int32_t err_len) {
    if (!path || !supply || (n_arcs > 0 && (!tail || !head || !lower || !cap || !cost))) return MCF_E_BAD_ARG;
    for (int64_t v = 0; v < n_nodes; ++v) supply[v] = 0;
    int64_t i = 0;
    return dimacs_walk(
        path, err, err_len,
        [&](int64_t nn, int64_t mm, const std::string& where) {
            return (nn == n_nodes && mm == n_arcs) ? 0 : dimacs_fail(err, err_len, where + "counts differ from mcf_dimacs_scan");
        },
        [&](int64_t id, int64_t sup, const std::string& where) {
            if (id < 1 || id > n_nodes) return dimacs_fail(err, err_len, where + "node id outside [1, " + std::to_string(n_nodes) + "]");
            supply[id - 1] = sup;
            return 0;
        },
        [&](int64_t t, int64_t h, int64_t lo, int64_t cp, int64_t c, const std::string& where) {
            if (t < 1 || t > n_nodes || h < 1 || h > n_nodes)
                return dimacs_fail(err, err_len, where + "Arc references node IDs outside the expected range [1, " + std::to_string(n_nodes) + "]");
            if (i >= n_arcs) return dimacs_fail(err, err_len, where + "more arc descriptors than the problem line announces");
            tail[i] = (int32_t)(t - 1); head[i] = (int32_t)(h - 1); lower[i] = lo; cap[i] = cp; cost[i] = c;
            ++i;
            return 0;
        });
}

void mcf_destroy(mcf_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_all(h);
    delete h;
}

}  // extern "C"
