/*
 * mcf.h -- C ABI of libmcf_hip.so, the MI355X (gfx950) network-simplex pivot engine.
 *
 * The reference (jeffreyhorn/network_flow_solver) is pure Python and has no FFI; its
 * seams are Python-level.  This library is what a ctypes stub
 * behind those seams binds:
 *
 *   reference seam (file:line under /root/reference/src/network_solver/)      entry point here
 *   -----------------------------------------------------------------------   ----------------
 *   NetworkSimplex.__init__: arc build, SoA mirror, initial tree
 *       simplex.py:99-265, 392-456, 619-730 ..................................  mcf_create
 *   NetworkSimplex.solve / _run_simplex_iterations / _pivot
 *       simplex.py:1109-1160, 1176-1425, 1446-1701 ...........................  mcf_solve
 *   result extraction  simplex.py:1703-1765 ..................................  mcf_get_result
 *   PricingStrategy.select_entering_arc  simplex_pricing.py:57-86, 97-137,
 *       310-357 and NetworkSimplex._select_entering_arc_vectorized
 *       simplex.py:528-617 ...................................................  mcf_price_once
 *   ProgressCallback cadence  simplex.py:1143-1154 ...........................  mcf_progress_cb
 *   UnboundedProblemError(entering_arc, reduced_cost)  exceptions.py:65-93 ...  MCF_ST_UNBOUNDED + stats.unbounded_arc
 *   warm start  simplex.py:740-1010, 1491-1532 ..............................  mcf_set_basis
 *   solving again after arc costs changed: the reference builds a new NetworkSimplex
 *       from the edited problem and passes solve(warm_start_basis=...)
 *       simplex.py:99-265, 1491-1532 .........................................  mcf_update_costs (the resident basis stays)
 *   solving again after supplies / demands / capacities changed: the reference builds a new NetworkSimplex from the edited
 *       problem and passes solve(warm_start_basis=...), which recomputes the tree flows and falls back to the cold start
 *       when one of them leaves its bounds  simplex.py:99-265, 905-1010, 1491-1532 ...  mcf_update_rhs (the resident basis stays or is repaired)
 *       the same edit re-optimised the way the algorithm wants -- the basis stays dual feasible, so DUAL pivots on the device
 *       drive the violated tree flows back inside their bounds (the reference has no dual simplex) ...  mcf_update_rhs_dual
 *   adding arcs to a solved problem (examples/incremental_resolving_example.py:222-266, scenario 4): the reference builds a new
 *       NetworkSimplex from the extended problem and warm-starts it  simplex.py:99-265, 1491-1532 ...  mcf_add_arcs (the resident basis stays)
 *   validate_flow / compute_bottleneck_arcs  utils.py:169-312 (conservation, bounds, arcs
 *       near capacity of a solution; the reference checks nothing on the dual side) ......  mcf_certify / mcf_bottlenecks
 *   UnboundedProblemError / status "infeasible" carry no witness in the reference (exceptions.py:65-93 names the entering
 *       arc, simplex.py:1600-1624 returns an empty flow): the ray and the cut that prove them ...  mcf_certify_ray / mcf_certify_cut
 *   "what if this cost changes": the reference answers by one re-solve per what-if (examples/sensitivity_analysis_example.py,
 *       examples/warm_start_example.py); the ranges inside which no re-solve pivots, for all arcs at once ...  mcf_cost_ranges
 *   "what if this supply / capacity changes": the reference predicts the objective from the duals and re-solves to see whether
 *       the prediction held (examples/sensitivity_analysis_example.py), and lists saturated arcs without a price or a range
 *       (utils.py:250-312); how far the prediction holds, and its exact rate ...  mcf_supply_ranges / mcf_capacity_ranges
 *   AdaptiveTuner.adapt_block_size  simplex_adaptive.py:98-151 and the
 *       periodic Devex reset  simplex.py:1370-1400 ..........................  inside mcf_solve (MCF_RULE_DEVEX_BLOCK)
 *   specialised pivot strategies  specialized_pivots.py:69-424, 452-527 .....  mcf_options.key_mode (+ arc_priority): row scan,
 *                                                                               min-cost scan, shortest-path / matching
 *                                                                               preference classes, max-flow capacity merit
 *   the benchmark runner's loop over instances
 *       benchmarks/runners/run_benchmark.py (one solve after the other) ......  mcf_solve_batch (one launch, one CU per instance)
 *   parse_dimacs_file  benchmarks/parsers/dimacs.py:77-286 ..................  mcf_dimacs_scan / mcf_dimacs_load
 *
 * Conventions: plain pointers and sizes only; integer return codes (0 = ok, < 0 =
 * MCF_E_*), never exceptions; the caller owns every buffer it passes; the library owns
 * device memory until mcf_destroy; one handle is not thread-safe, distinct handles are
 * independent (handles of small instances share a few pooled streams: their work is
 * serialised on the device, never mixed up).  All problem data are integers: the Python shim scales decimal input
 * (and applies the reference's lower-bound shift, simplex.py:413-428) before the call.
 *
 * There is NO CPU fallback: every compute entry point fails with MCF_E_NO_DEVICE when no
 * HIP device is usable.
 */
#ifndef MCF_H
#define MCF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCF_ABI_VERSION 3

/* return codes */
#define MCF_OK 0
#define MCF_E_BAD_ARG (-1)
#define MCF_E_NO_DEVICE (-2)
#define MCF_E_HIP (-3)
#define MCF_E_ALLOC (-4)
#define MCF_E_RANGE (-5)     /* value outside what the integer engine represents */
#define MCF_E_STATE (-6)     /* call not valid in the handle's current state */
#define MCF_E_INTERNAL (-7)

/* solve status (mcf_get_result) -- mapped by the shim onto the reference's strings
 * (data.py:269-322): optimal / infeasible / iteration_limit; unbounded becomes
 * UnboundedProblemError. */
#define MCF_ST_OPTIMAL 0
#define MCF_ST_INFEASIBLE 1
#define MCF_ST_ITERATION_LIMIT 2
#define MCF_ST_UNBOUNDED 3

/* pricing rules */
#define MCF_RULE_DANTZIG_FULL 0   /* full-scan most-violating arc (simplex_pricing.py:97-137) */
#define MCF_RULE_DEVEX_BLOCK 1    /* round-robin block search, merit rc^2/w, deferred weight update
                                     (simplex_pricing.py:310-357, 271-292), block-size tuner (simplex_adaptive.py:98-151),
                                     weights reset every 64 basis swaps (simplex.py:1370-1400) */
#define MCF_RULE_CANDIDATE_LIST 2 /* full Dantzig sweep keeps one candidate per pricing workgroup; the following
                                     pivots re-price only that list (simplex_pricing.py:375-542, 419-456) */

/* State of the pricing rules -- what decides WHICH arc enters next, complete enough to implement from (DESIGN.md section 4 has
 * the same text with its reasons; tests/rule_reference.py is written from it and shares no code with the engine).
 *
 * Engine arc order.  Arcs are bucketed by head: bucket x = head / ceil(n / 8), x = 0 .. 7; inside a bucket they are ordered by
 *   tail, equal tails in the caller's order.  bucket_off[x] = engine index of the first arc of bucket x.
 * Violation.  viol = -state * (cost + pi[tail] - pi[head]), state +1 at the lower bound (a FORWARD candidate), -1 at capacity
 *   (BACKWARD), 0 basic; an arc is eligible when viol > 0.
 *
 * MCF_RULE_DEVEX_BLOCK
 *   Granules: granule g of bucket x = the engine arcs bucket_off[x] + len_x * g / 64 .. bucket_off[x] + len_x * (g + 1) / 64 (integer
 *     division, len_x = arcs of the bucket), g = 0 .. 63.  A block of bg granules, block k, = granules k * bg .. min(k * bg + bg, 64)
 *     of EVERY bucket; num_blocks = ceil(64 / bg).  mcf_stats.arcs_priced grows by the arcs of the block at every pass.
 *   Start: block 0, every weight 1, bg = clamp((bs * 64 + m / 2) / m, 1, 64) with bs = block_size when given, else the automatic
 *     m / 4 (m < 1 000), m / 8 (m < 10 000), m / 16, at least 1.  The tuner is on exactly when the size is automatic
 *     (devex_tuner 1 / -1: on / off whatever block_size says); its cap is max(bg, min(64, 16 384 * 64 / m)) granules.
 *   A pass prices the current block: merit = (double)viol * (double)viol / (double)w in IEEE double, w the arc's float32 weight.
 *     The largest merit enters; among equal merits a backward arc before a forward one (forward wins only when strictly greater),
 *     then the lowest caller's index.  No eligible arc: empty_blocks += 1, next block (cyclically), and optimal once
 *     empty_blocks >= num_blocks.  Otherwise empty_blocks = 0 and -- unless devex_stay -- the block index advances (cyclically)
 *     before the pivot is made.
 *   After the pivot, in this order:
 *     (1) a basis swap (the leaving arc is not the entering arc) with 64 swaps counted: RESET, count = 0 (that swap is not
 *         counted); any other swap: count += 1.  Bound flips never count;
 *     (2) no reset so far: with 1 024 weights set since the last reset (an arc counts every time it enters): RESET (early; the swap
 *         count stays); else the entering arc's weight = the tree arcs on its cycle (at least 1), the other weights stay;
 *     (3) RESET = every weight reads 1.0 again from this pivot on (the entering arc's included), the block index is 0;
 *     (4) tuner, when on: the pivot counts, and counts as degenerate when it moved no flow OR was a bound flip.  With at least 50
 *         pivots since the last adaptation: more than 30 % degenerate: bg = max(bg, min(max(bg * 3 / 2, bg + 1), cap)); fewer than
 *         10 %: bg = max(bg * 3 / 4, 1); the counts start over either way.  A changed bg changes num_blocks; a block index that
 *         is no longer below num_blocks wraps to 0.
 * MCF_RULE_CANDIDATE_LIST
 *   The pricing grid has 8 * k workgroups, k = clamp(ceil(price_blocks / 8), 1, 256) (automatic: k = ceil(m / 8 / 2 048), same
 *     clamp); engine arc e of bucket x belongs to workgroup (((e >> 2) - (bucket_off[x] >> 2)) >> 8) mod k of that bucket: runs of
 *     1 024 arcs dealt out in turn.  minor_cap = clamp(k, 3, 32).  The fused LDS loop has no grid: there k = 1 whatever
 *     price_blocks says.
 *   A full sweep (arcs_priced += m) keeps, per workgroup, its eligible arc of the largest violation, ties to the lowest caller's
 *     index; the best of these -- same order -- enters.  None: optimal; only a full sweep ever says so.  Then up to minor_cap
 *     minor pivots: each re-prices the 8 * k list entries (arcs_priced += 8 * k) under the current potentials and states -- an
 *     entry that has become basic or is no longer eligible counts as absent, one that is eligible again takes part -- and the best
 *     enters.  A list without an eligible arc ends the period early, without a pivot; the next pass is a full sweep. */

/* "uncapacitated" marker accepted in cap[] (besides any value >= 2^60) */
#define MCF_CAP_INF (-1)

typedef struct mcf_handle mcf_handle;

typedef struct mcf_options {
    int32_t abi_version;     /* MCF_ABI_VERSION */
    int32_t device;          /* HIP device ordinal; -1 = current device */
    int32_t rule;            /* MCF_RULE_* */
    int32_t batch_pivots;    /* pivots enqueued per host round trip (0 = default 64) */
    int32_t use_graph;       /* 1 = replay a captured hipGraph of batch_pivots pivots */
    int32_t profile;         /* 1 = bracket every kernel with HIP events (no graph), fills *_ms */
    int64_t block_size;      /* Devex block size; 0 = auto (simplex_adaptive.py:89-96) */
    int64_t shard_rank;      /* multi-GPU: this handle prices shard shard_rank of shard_count */
    int64_t shard_count;     /*   (0 or 1 = all arcs); a shard is 1/shard_count of every XCD head bucket */
    int32_t price_blocks;    /* pricing grid size; 0 = auto */
    int32_t no_fused;        /* 1 = never use the fused LDS-resident kernel for small instances */
    int32_t no_rcache;       /* 1 = never keep reduced costs resident: always price by gathering potentials */
    int32_t cycle_scan;      /* cycle search: 0 = auto, -1 = always climb parent pointers, k >= 1 = climb k - 1 round
                                trips, then finish by the position-space scan (1 = scan only) */
    int32_t mid_loop;        /* persistent single-workgroup pivot loop for mid-size instances (k_solve_mid):
                                0 = auto (by size and rule), -1 = never, 1 = whenever the handle allows it */
    int32_t full_sweeps;     /* incremental Dantzig / candidate-list sweeps (a pricing workgroup whose arcs have not changed since
                                it last swept them keeps its candidate): 0 = auto (from 4 M arcs), 1 = never, -1 = always */
    int32_t devex_tuner;     /* Devex block-size tuner (simplex_adaptive.py:98-151): 0 = auto (on when block_size is 0, as in the
                                reference; off for a caller-given block size), 1 = on, -1 = off */
    int32_t devex_stay;      /* Devex block advance: 0 = cyclic (next block after every pivot), 1 = stay on a block until it holds
                                no eligible arc (the reference's loop, simplex_pricing.py:325-355; needs the tuner to converge) */
    int32_t forward_first;   /* 1 = Dantzig / candidate-list keys rank every forward candidate above every backward one: the
                                reference's min-cost entering rule for assignment problems (specialized_pivots.py:191-223) followed
                                by its general pricing for what is left (simplex.py:1061-1064).  The row-scan rule it uses for
                                transportation problems (specialized_pivots.py:69-117) IS MCF_RULE_DANTZIG_FULL. */
    int32_t compressed_keys; /* Dantzig / candidate-list grid sweeps over 4-byte key codes (one per arc, kept exact next to the resident
                                reduced costs) instead of 8 B reduced cost + 1 B state: 0 = auto (full-sweep Dantzig handles from 4 M arcs on, where the
                                sweep is bandwidth-bound and read whole), 1 = on, -1 = off */
    int32_t vkey_half_log2;  /* test hook: log2 of the half width of a code level (0 = 28); small values force the exact-compare path */
    int32_t climb_depth;     /* cycle search: end points no deeper than this are climbed outright whatever cycle_scan says
                                (0 = auto: 3 up to 32 768 nodes, 8 above; -1 = never) */
    int32_t overlap_update;  /* captured graphs in which the pricing of pivot t+1 runs beside the tree permutation of pivot t (it needs
                                only the reduced-cost half of the update): 1 = on, 0 / -1 = off.  Same pivot sequence.  Measured
                                slower at every size (two cross-queue edges per pivot cost ~12 us on this stack;
                                profiles/r02_ab_overlapped_graph.txt), so auto never picks it: kept as an A/B switch. */
    int32_t key_mode;        /* key variant of the Dantzig / candidate-list sweep = the reference's specialised entering rules
                                (specialized_pivots.py:69-424, dispatch :452-527) as variants of the one kernel:
                                0 = plain violation (also the transportation row scan :69-117; forward_first = 1 selects 1),
                                1 = forward candidates first (assignment, :191-223),
                                2 = candidates flagged in arc_priority first (shortest path :338-424, bipartite matching :233-281),
                                3 = capacity x violation (max flow, :284-335).  Not with MCF_RULE_DEVEX_BLOCK. */
    const int8_t* arc_priority; /* key_mode 2: one byte per arc, caller's order; bit 0 = preferred as a forward candidate (flow rises
                                from the lower bound), bit 1 = preferred as a backward candidate.  Read during mcf_create only. */
    int32_t tree_blocks;     /* layout of the spanning tree's preorder: 0 = auto (blocked preorder list from 200 000 nodes on), -1 = dense
                                array, k in 2..10 = blocked list with blocks of 2^k slots.  The blocked list re-hangs a subtree in
                                O(subtree + block) element moves instead of shifting every position between its old and its new
                                place (replaces the per-pivot BFS rebuild basis.py:82-125 and _update_tree_sets simplex.py:1103-1107);
                                same logical preorder, same pivots.  Handles of the persistent loops (pricing_mode 2 / 3, mid_loop = 1)
                                keep the dense array. */
    int32_t tree_pool;       /* blocked list: spare blocks per arena (0 = auto: 1.5 x the dense count; -1 = none, so that every pivot
                                rewrites the whole list -- a test hook) */
    int32_t rc_drop;         /* resident reduced costs are given up in mid-solve -- pricing then gathers the potentials, as with no_rcache --
                                once the re-hung subtrees average more than this many nodes over a batch of pivots: from there on the
                                patch of the incident arcs' reduced costs costs more per pivot than the dearer sweeps.  0 = auto
                                (from 100 000 nodes on: candidate list 384, Devex 1 500; else never), -1 = never, k > 0 = that threshold (candidate
                                list and Devex; the Dantzig rule sweeps every arc on every pivot and never drops).  Same pivots. */
    int32_t pivot_run;       /* candidate-list handles on the blocked list: a list period is one sweep + this many pairs of (k_pivot_run:
                                pivots back to back in ONE workgroup, each followed by its update in place, until an update is too large
                                for one workgroup or the list is used up; k_update_bpl: that update on the grid).  0 = off (measured
                                slower than the pair shape at 1M/16M: 30.9-35.7 K against 41.1 K pivots/s; the
                                environment variable MCF_PIVOT_RUN=k turns it on for an A/B), k > 0 = k pairs (the handle goes back
                                to one k_pivot per slot once its run launches end after fewer than three pivots on average).
                                Same pivots in the same order. */
} mcf_options;

typedef struct mcf_stats {
    int64_t pivots;           /* FlowResult.iterations (degenerate pivots included) */
    int64_t degenerate;       /* theta == 0 */
    int64_t bound_flips;      /* leaving arc == entering arc */
    int64_t arcs_priced;      /* sum over pricing passes of the arcs the pass covers */
    int64_t nodes_moved;      /* preorder positions rewritten by the apply pass */
    int64_t subtree_nodes;    /* sum of re-hung subtree sizes */
    int64_t cycle_arcs;       /* sum of cycle lengths */
    int64_t batches;          /* host round trips */
    int64_t unbounded_arc;    /* entering arc when status is MCF_ST_UNBOUNDED, else -1 */
    int64_t unbounded_rc;     /* its reduced cost in the push direction (< 0) */
    double solve_seconds;     /* wall time inside mcf_solve */
    double price_ms;          /* with options.profile: summed kernel durations */
    double pivot_ms;
    double apply_ms;
    int64_t price_launches;
    int64_t pivot_launches;
    int64_t apply_launches;
    int64_t price_bytes;      /* compulsory bytes of one pricing launch of this handle's sweep kernel: 4 B/arc (k_price_v, key codes),
                                 9 B/arc (k_price_rc; 13 Devex), or SURVEY 8d's 13 B/arc + 8 B/node (k_price gather; 17 Devex) */
    int64_t artificial_flow;  /* flow still on artificial arcs (> 0 at optimality = infeasible, simplex.py:1573-1624);
                                 -1 when mcf_get_result was asked for neither status, objective nor flow */
    int64_t pricing_mode;     /* 0 = gather sweep (k_price), 1 = resident reduced costs (k_price_rc + k_rcupd),
                                 2 = fused LDS-resident pivot loop (k_solve_small),
                                 3 = persistent single-workgroup loop over global memory (k_solve_mid) */
    int64_t cycle_scans;      /* pivots whose cycle was completed by the position-space scan */
    int64_t scan_rounds;      /* chunk iterations of those scans */
    int64_t arcs_swept;       /* arcs whose reduced cost the grid sweeps actually read (<= arcs_priced with incremental pricing) */
    double loop_ms;           /* persistent pivot loops (pricing_mode 2, and 3 outside a graph): summed kernel durations, by HIP
                                 events on the engine's stream around every launch */
    int64_t loop_launches;    /* ... and the number of launches (one launch runs many pivots) */
    int64_t sweep_variant;    /* which grid sweep the handle launches: bit 0 = 4-byte key codes (k_price_v), bit 1 = non-temporal
                                 loads (k_price_v<.., true>), bit 2 = incremental (clean workgroups keep their candidate) */
    int64_t tree_blocks;      /* log2 of the block size of the blocked preorder list, 0 = dense preorder array */
    int64_t tree_rebuilds;    /* blocked list: pivots whose update rewrote the whole list densely (the block pool had run out) */
    int64_t rc_dropped_at;    /* pivot count at which the handle gave up its resident reduced costs (mcf_options.rc_drop), 0 = it has not */
    int64_t run_pairs;        /* (k_pivot_run, k_update_bpl) pairs per list period right now (mcf_options.pivot_run), 0 = one k_pivot per slot */
    int64_t run_left_at;      /* pivot count at which the handle went back to one k_pivot per slot, 0 = it has not */
    int64_t small_narrow;     /* fused LDS loop (pricing_mode 2): 1 = the handle's last launch was told that every reduced cost of the
                                 instance fits 32 bits (mcf_small_narrow_ok with the big-M of that moment; its Dantzig / candidate-list
                                 sweep then prices with 32-bit keys), 0 = 64-bit keys (the range does not fit, or MCF_SMALL_NARROW=0),
                                 or no launch of that loop yet.  Same pivots either way. */
} mcf_stats;

/* The range test behind mcf_stats.small_narrow, a pure function of the instance: with big-M = big_m and max|cost| =
 * max_abs_cost (big_m >= (max_abs_cost + 1) * (n + 2), as mcf_create forms it), every reduced cost, violation and potential
 * shift of a solve stays within *bound (may be NULL) = 4 * big_m - 5 * max_abs_cost - 1 in magnitude (derivation:
 * csrc/mcf_host.h); returns 1 when that fits int32, else 0.  Needs no device. */
int mcf_small_narrow_ok(int64_t big_m, int64_t max_abs_cost, int64_t* bound);

/* Called from mcf_solve every cb_interval pivots (simplex.py:1143-1154).
 * Return non-zero to stop the solve (status becomes MCF_ST_ITERATION_LIMIT). */
typedef int (*mcf_progress_cb)(void* user, int64_t pivots, int64_t max_pivots, double elapsed_seconds);

/* Fill *opt with defaults. */
void mcf_default_options(mcf_options* opt);

/* ---- Numeric domain.  Everything is exact integer arithmetic; mcf_create checks what follows on the host, before
 * anything reaches a device, and refuses an instance outside it with MCF_E_RANGE and a message (mcf_last_error(NULL)).
 *   sizes       n >= 1, m >= 0, m + n < 2^30.
 *   costs       |cost| <= INT32_MAX = 2^31 - 1 (negative and zero costs included; -2^31 is refused), and
 *               big-M = (max|cost| + 1) * (n + 2) < 2^44: the cost of an artificial arc, above any simple path's cost.
 *               INT32_MAX is therefore admissible up to n = 8 189.  Potentials (+-big-M plus the cost of a tree path) stay below
 *               2 * big-M < 2^45 in magnitude and reduced costs below 4 * big-M < 2^46, which is what leaves bit 61 free for the key variants and lets the Devex
 *               merit rc^2 / w be formed in double precision (convert, multiply, divide; never contracted).
 *   capacities  int64.  0 <= cap < 2^60 is a bound and is honoured exactly (2^60 - 1 included); cap < 0 (MCF_CAP_INF)
 *               or cap >= 2^60 means uncapacitated.  2^60 is also the ratio test's "no bound": a pivot whose cycle has
 *               no bound at all ends the solve as MCF_ST_UNBOUNDED.
 *   supplies    int64, summed in 128 bits: sum(supply) must be 0, and the sum of the POSITIVE supplies must stay below
 *               2^60.  That sum bounds the flow of every artificial arc at every pivot (a pivot cycle passes the root
 *               through one artificial arc in each sense, so their total never grows beyond the start basis'), and an
 *               artificial arc at 2^60 would read as unbounded.  The limit is 2^60 itself, not something tighter: below
 *               it every residual the ratio test compares is < 2^60, and flow + residual < 2^61 cannot overflow.
 *   flows       a capped arc never carries more than its capacity.  An UNCAPACITATED arc on a negative-cost cycle
 *               closed by capped arcs carries up to the sum of those capacities: keeping that below 2^60 is the
 *               caller's part (it cannot be checked without solving).
 *   objective   sum(flow * cost) as an exact 128-bit integer, handed over as two 64-bit halves (mcf_get_result);
 *               |objective| < m * 2^60 * 2^31 < 2^121. */

/* Build the device-resident problem: arc SoA, potentials, preorder spanning tree with the
 * all-artificial start basis.  n = real nodes (ids 0..n-1), m = arcs, lower bounds already
 * shifted out.  cap[i] < 0 or >= 2^60 means uncapacitated.  sum(supply) must be 0 and the positive
 * supplies must add up to less than 2^60.  |cost| must fit int32 (and big-M stay below 2^44, see
 * "Numeric domain" above) and m + n must stay below 2^30; outside: MCF_E_RANGE. */
int mcf_create(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost,
               const int64_t* cap, const int64_t* supply, const mcf_options* opt, mcf_handle** out);

/* Pivot until optimal / unbounded / max_pivots more pivots were made (max_pivots < 0:
 * the reference's default budget max(100, 20 * (m + n)), simplex.py:1470).
 * A verdict is final: on a handle whose status is already optimal, infeasible or unbounded the call is a no-op that makes no
 * pivot and leaves status, counters (mcf_stats.pivots, unbounded_arc, ...) and every array as they are; only an iteration
 * limit is resumed.  mcf_reset, mcf_set_basis, mcf_update_costs, mcf_update_rhs and mcf_add_arcs are what put such a handle back to "running". */
int mcf_solve(mcf_handle* h, int64_t max_pivots, mcf_progress_cb cb, void* user, int64_t cb_interval);

/* Solve `count` INDEPENDENT instances side by side: one persistent workgroup (one CU) per handle, each running its whole
 * solve as mcf_solve would (same pivot sequence, same budget rule; no progress callback), all in one launch per engine path.
 * The reference solves instances one after the other on one core (benchmarks/runners/run_benchmark.py; its published
 * per-instance figures are all for <= 4 096 nodes): a single such instance can only ever occupy one CU of 256, a batch
 * fills the chip.  Every handle must run as one persistent workgroup -- the fused LDS path (mcf_stats.pricing_mode == 2:
 * about <= 300 nodes / 2 500 arcs) or the persistent loop over global state (pricing_mode == 3; mcf_options.mid_loop = 1
 * asks for it at any size; a candidate-list loop then does its full sweeps itself) -- on the same device; max_pivots: one budget per handle (< 0: the
 * reference's default) or NULL for the default everywhere; kernel_ms (optional) <- duration of the launches.  Results per
 * handle through mcf_get_result as usual. */
int mcf_solve_batch(mcf_handle* const* handles, int32_t count, const int64_t* max_pivots, double* kernel_ms);

/* Copy the solution out.  Any pointer may be NULL.  objective_hi_lo[0..1] = high and low
 * 64 bits of the exact 128-bit sum(flow*cost); flow[m]; potential[n] (root excluded);
 * in_tree[m]. */
int mcf_get_result(mcf_handle* h, int32_t* status, int64_t* objective_hi_lo, int64_t* flow,
                   int64_t* potential, int8_t* in_tree, mcf_stats* stats);

/* One pricing pass over arcs [start, end) (caller's arc indices) with the current potentials,
 * without pivoting: the kernel-level parity hook.  Ties go to the lowest arc index.  *arc = -1 when no arc is eligible; *dir = +1 forward /
 * -1 backward; *key = violation |rc| (Dantzig) or the f64 merit's bit pattern (Devex). */
int mcf_price_once(mcf_handle* h, int32_t rule, int64_t start, int64_t end, int64_t* arc, int32_t* dir,
                   int64_t* key);

/* Back to the all-artificial start basis (flows, potentials, tree, counters). */
int mcf_reset(mcf_handle* h);

/* Warm start (NetworkSimplex._apply_warm_start_basis, simplex.py:740-903, and _recompute_tree_flows,
 * :905-1010): restart from the caller's basis instead of the all-artificial one.  in_tree[m] marks the basic
 * arcs (they must form a forest; every component gets one artificial arc to the root, as in the reference);
 * at_upper[m] (may be NULL) marks non-basic arcs sitting at their capacity rather than at zero (the reference
 * keeps no such information in a Basis and starts them at zero).  Tree flows are recomputed from conservation
 * with the handle's supplies / capacities.  Returns MCF_OK, or MCF_E_STATE when the basis cannot be used (cycle,
 * empty, flows outside the bounds): the handle is then at the cold start and can be solved as usual -- the
 * reference's fall-back (simplex.py:1527-1531).  Counters are reset either way. */
int mcf_set_basis(mcf_handle* h, const int8_t* in_tree, const int8_t* at_upper);

/* Re-optimise after arc costs changed: arc[i] (caller's arc index) now costs new_cost[i]; the basis the handle holds stays.
 * Flows, arc states and the tree do not depend on costs, so that basis stays primal (and strongly) feasible under any cost
 * vector: only the potentials below a changed tree arc move, and after them the reduced costs and key codes.  All of it is
 * done on the device, on the arrays that are already there -- no new handle, no upload of the instance, no host walk of the
 * tree -- and the next mcf_solve simply goes on pivoting from that basis.
 *   valid      between solves in any state of the handle (fresh, after mcf_reset / mcf_set_basis, after a solve that ended
 *              with any status), on every engine path, tree layout, rule and key_mode.  Duplicate indices: the LAST entry
 *              wins (resolved on the host).  Handles with shard_count > 1: MCF_E_STATE.
 *   errors     MCF_E_BAD_ARG: null handle, count < 0, null arrays with count > 0, an index outside [0, m).  MCF_E_RANGE: a
 *              cost outside "Numeric domain" above (|cost| > INT32_MAX, or big-M would reach 2^44).  Everything is checked
 *              before anything changes: after either error the handle is exactly as it was.
 *   big-M      grows in the same call when a new cost needs it ((max|cost| + 1) * (n + 2), as in mcf_create) -- every
 *              artificial arc touches the root, so that is a cost change on the tree arc of every root child that still hangs
 *              on one -- and never shrinks.
 *   afterwards the handle is what mcf_create with the new costs followed by an installation of this basis would give:
 *              flows, states, parent / pred_arc / size / pos / order / depth / psize unchanged; the root's potential
 *              unchanged and pi[child] - pi[parent] = +-cost(pred arc) on every tree arc; resident reduced costs and key
 *              codes (where the handle keeps them; a handle that dropped them stays dropped) exact for every arc.  The
 *              solve status is back to "running"; mcf_stats.pivots and the other counters keep counting (mcf_solve(h, k)
 *              means k MORE pivots).  Everything derived for pricing starts over: the candidate list and its cache are
 *              emptied, every pricing workgroup of an incremental sweep is due again, the Devex weights are 1.0, the
 *              block cursor and the block-size tuner are at their start values.  A later mcf_reset / mcf_set_basis and
 *              the objective of mcf_get_result use the new costs. */
int mcf_update_costs(mcf_handle* h, int64_t count, const int64_t* arc, const int64_t* new_cost);

/* Re-optimise after supplies / demands and arc capacities changed: node[i] now supplies new_supply[i], arc[i] (caller's arc
 * index) now has capacity new_cap[i] (mcf_create's convention: < 0 or >= 2^60 = uncapacitated); both kinds of change in one
 * call, so that a combined edit is one pass.  It replaces the reference's only way to do this -- a new NetworkSimplex from
 * the edited problem plus solve(warm_start_basis=...), simplex.py:99-265, 905-1010, 1491-1532, which uploads nothing because
 * it has nothing resident, walks the tree on the host and drops the basis altogether ("basis incompatible with the current
 * supplies / capacities", :1527-1531) as soon as ONE tree flow leaves its bounds.
 *   what stays   flows and states of non-basic arcs do not depend on supplies; reduced costs depend on neither supplies nor
 *                capacities.  A non-basic arc at capacity follows its new capacity (and goes back to its lower bound when
 *                the new capacity is 0 or none: upper_moved counts both).  Tree flows are subtree sums of node balances
 *                (supply minus outflow plus inflow of the non-basic arcs, 128-bit), and a subtree is a contiguous range of
 *                the preorder: one gather over the node -> arc adjacency, one device-wide prefix sum over preorder positions
 *                (dense preorder array and blocked preorder list alike), one pass that writes the tree flows and takes the
 *                census.  flow[m] and the tree are never downloaded for this.
 *   path 0       no tree arc is out of bounds (flow < 0, > capacity, or magnitude >= 2^60) and no basic arc sits on a bound
 *                pointing the wrong way (zero flow away from the root, full flow towards it): the basis stays.  An
 *                artificial tree arc whose flow changed sign turns round (art_flips); only then do potentials (below it, by
 *                -+2 big-M), reduced costs and key codes change, rebuilt as mcf_update_costs rebuilds them.  A handle that
 *                was optimal and takes path 0 without a flip is optimal again: the next mcf_solve makes 0 pivots.
 *                mcf_supply_ranges / mcf_capacity_ranges say in advance which single edits take this path (their contract below).
 *   path 1       otherwise the states and the node records (not the flows) come down and the basis is repaired on the
 *                host at mcf_set_basis cost: every tree arc whose flow left its bounds becomes non-basic at the bound it
 *                violated, every wrong-way arc at the bound it sits on; each such subtree hangs on the root by its
 *                artificial arc, which carries what the cut arc no longer can (arcs_cut real arcs leave the basis, in
 *                repair_rounds sweeps over the tree).  The result is a strongly feasible basis with a few subtrees on big-M
 *                arcs, which the primal pivots of the next mcf_solve drive out.
 *   path 2       the repair refuses (a flow of 2^60 or more on an uncapacitated or artificial arc): cold start with the new
 *                data, as mcf_reset.
 *   valid        between solves in any state of the handle (fresh, mid-solve after an iteration limit, optimal, infeasible,
 *                unbounded), on every engine path, tree layout, rule and key_mode, and on handles that dropped their
 *                resident reduced costs.  Duplicate indices: the LAST entry wins.  Handles with shard_count > 1: MCF_E_STATE.
 *   errors       MCF_E_BAD_ARG: null handle, a negative count, null arrays with a positive count, an index outside [0, n)
 *                / [0, m).  MCF_E_RANGE: the new supply vector does not sum to 0 (128-bit sum) or its positive part reaches
 *                2^60.  Everything is checked before anything changes: after either error the handle is exactly as it was.
 *   afterwards   all three paths return MCF_OK and *out (may be NULL) says which one ran.  The solve status is back to
 *                "running"; mcf_stats.pivots and the other counters keep counting on every path.  Everything derived for
 *                pricing starts over as after mcf_update_costs.  A later mcf_reset / mcf_set_basis, mcf_certify and the
 *                objective of mcf_get_result use the new data. */
typedef struct mcf_rhs_report {
    int64_t path;             /* 0 = basis kept on the device, 1 = basis repaired (host), 2 = cold start */
    int64_t tree_violations;  /* tree arcs out of bounds after the recomputation (census on the device) */
    int64_t wrong_way;        /* basic arcs on a bound pointing the wrong way (strong feasibility) */
    int64_t arcs_cut;         /* real arcs the repair took out of the basis (path 1) */
    int64_t repair_rounds;    /* rounds of the repair loop (path 1) */
    int64_t art_flips;        /* artificial tree arcs whose direction turned round */
    int64_t upper_moved;      /* non-basic arcs at capacity that followed their new capacity */
    double  device_ms;        /* HIP events round the device passes */
} mcf_rhs_report;

int mcf_update_rhs(mcf_handle* h,
                   int64_t n_sup, const int64_t* node, const int64_t* new_supply,
                   int64_t n_cap, const int64_t* arc,  const int64_t* new_cap,
                   mcf_rhs_report* out /* may be NULL */);

/* mcf_update_rhs with a dual simplex phase on the device in front of path 1.  A supply / capacity edit leaves the resident basis
 * DUAL feasible (reduced costs depend on neither) while some tree flows leave their bounds; instead of cutting every violated arc
 * out on the host and driving big-M arcs back out with primal pivots, dual pivots repair the flows on the arrays that are resident.
 *   before       argument checks, duplicate rule, errors and the device passes up to the census are mcf_update_rhs's own (one
 *                code path).  The census stores the violating tree flows too (magnitude below 2^60), for the phase to work on.
 *   the phase    runs where the census finds tree_violations > 0 and nothing below forbids it; otherwise ended = 3 and the call
 *                IS mcf_update_rhs.
 *   afterwards   tree flows and census are recomputed by the same passes, and the call continues exactly as mcf_update_rhs
 *                does after its census -- path 0, 1 or 2 on the basis the phase left.  *out is that second census (upper_moved:
 *                the first).  Every violation cleared and no wrong-way arc: path 0, an optimal handle is optimal again and the
 *                next mcf_solve makes 0 pivots.  Otherwise the repair of path 1 picks up what is left: the phase is best effort,
 *                the call always correct.  mcf_stats.pivots, degenerate, bound_flips and arcs_priced do not move in the phase.
 *   the rule     exact integers throughout: rc = cost + pi[tail] - pi[head], slack = state * rc (>= 0 on every non-basic arc).
 *     leaving    candidates: the tree arcs of the nodes 0 .. n-1 (artificial ones included).  violation = -flow when flow < 0,
 *                flow - cap when the arc is capped and flow > cap.  The LARGEST violation leaves, ties to the lowest node; it
 *                leaves at the bound it violated (state +1 at 0, -1 at capacity).
 *     entering   q = the leaving arc's child node, S = the subtree of q (interval test on logical preorder positions, both tree
 *                layouts).  When the arc carries too much from child to parent (an up arc over capacity, a down arc below 0) S
 *                must EXPORT: candidates are the non-basic real arcs with cap != 0 at state +1 with tail in S and head outside,
 *                or at state -1 with head in S and tail outside.  Otherwise S must import: the two classes mirrored.  The
 *                LEAST slack enters, ties to the lowest caller's index.  No candidate: the edited instance needs artificial
 *                flow across that cut; the phase stops (ended = 1).
 *     pivot      the entering arc is pushed in its own direction by delta = the violation along the engine's route (second ->
 *                join -> first -> arc): the leaving arc lands exactly on its bound; other cycle arcs -- the entering arc
 *                included -- may leave theirs and are later leaving candidates.  T2 = S re-hangs on the entering arc; the
 *                potentials of S shift by sigma = -rc when the arc's tail is in S, +rc otherwise, which zeroes the entering
 *                arc's reduced cost and lowers every candidate's slack by the least one: dual feasibility is kept by construction.
 *     the end    a closed arc (cap == 0) is no candidate, so nothing keeps its slack from turning negative; its flow is 0 at
 *                either bound, and when the phase ends every such arc takes the state its reduced cost asks for (state =
 *                -state, no flow moves).  With that every non-basic arc has slack >= 0 again.
 *     magnitudes a pivot adds a violation to a flow; the phase stops (ended = 4) before a pivot when a tree flow or the violation
 *                reaches 2^61 in magnitude, so no sum reaches 2^62.  Flows of 2^60 or more after the first census: reason 5.
 *   options      max_pivots < 0: 163 * violations_before (twice the largest ratio of dual pivots per violation measured, 81.45).
 *                enter_walk: 0 = auto (the subtree's adjacency is walked when it has <= 64 nodes, else the arcs are swept),
 *                -1 = always the sweep, k > 0 = walk when |S| <= k.  Both searches choose the same arc.
 *   log          four words per dual pivot: leaving arc (caller's index; m + v for the artificial arc of node v), entering arc
 *                (caller's index), delta, slack.  The first log_cap pivots are kept; log may be NULL with log_cap 0.
 *   valid        where mcf_update_rhs is valid; the phase itself runs on grid handles (both tree layouts, with or without
 *                resident reduced costs or key codes, every rule and key_mode).  shard_count > 1: MCF_E_STATE. */
typedef struct mcf_dual_options {
    int64_t max_pivots;   /* < 0 = default budget */
    int32_t enter_walk;   /* entering search: 0 = auto, -1 = always the arc sweep, k > 0 = walk the subtree's adjacency when it has <= k nodes */
    int32_t reserved;
} mcf_dual_options;

typedef struct mcf_dual_report {
    int64_t ended;              /* 0 = no violation left, 1 = a violated arc has no entering arc across its cut, 2 = budget exhausted,
                                   3 = not attempted (reason), 4 = magnitude limit */
    int64_t reason;             /* ended == 3: 1 = no violations, 2 = the handle runs as a persistent loop (pricing_mode 2 or 3),
                                   3 = basis not dual feasible (a real non-basic arc has state * rc < 0 after the edit; an arc at
                                   capacity whose capacity went to 0 or none can cause it), 4 = an artificial tree arc turned round
                                   (art_flips > 0), 5 = a tree flow of magnitude 2^60 or more */
    int64_t dual_pivots;
    int64_t violations_before;  /* tree_violations of the first census */
    int64_t violations_after;   /* ... of the census after the phase */
    int64_t wrong_way_after;
    int64_t sweeps, walks;      /* pivots whose entering arc came from the arc sweep / the adjacency walk */
    int64_t log_written;        /* pivots in log */
    double  device_ms;          /* HIP events round the phase */
} mcf_dual_report;

int mcf_update_rhs_dual(mcf_handle* h,
                        int64_t n_sup, const int64_t* node, const int64_t* new_supply,
                        int64_t n_cap, const int64_t* arc,  const int64_t* new_cap,
                        const mcf_dual_options* opt /* NULL = defaults */,
                        int64_t* log, int64_t log_cap,
                        mcf_rhs_report* out /* may be NULL */, mcf_dual_report* dual_out /* may be NULL */);

/* Add arcs to the resident handle: `count` new arcs tail[i] -> head[i] with cost[i] and cap[i] (mcf_create's conventions;
 * arc_priority[i] as in mcf_options.arc_priority for key_mode 2, NULL = 0).  New arc i gets the caller's index m + i, m the arc
 * count before the call.  A new arc enters non-basic at its lower bound with flow 0, so flows, potentials, the tree and every
 * existing reduced cost stay exactly as they are and the basis stays primal and strongly feasible: what has to happen is a
 * re-layout.  Engine order is a total order (head bucket, tail, caller's index); the new arcs belong inside it, and every
 * per-arc array, the node -> arc adjacency and the nodes' pred words follow.  That merge of two sorted sequences runs on the
 * device as streaming passes over the arrays that are already there; only the new arcs cross the bus (sorted on the host,
 * uploaded with their keys and the sorted list of their 2 * count end points), and nothing of size m comes down.  It replaces
 * a new mcf_create of the extended instance plus mcf_set_basis, which uploads the whole instance, walks the tree on the host
 * and throws the resident reduced costs, key codes and the blocked preorder list away.  Removing an arc needs no call of its
 * own: capacity 0 through mcf_update_rhs closes it and keeps every index.
 *   valid        between solves in any state of the handle (fresh, mid-solve after an iteration limit, optimal, infeasible,
 *                unbounded), on both tree layouts, every rule and key_mode, handles that dropped their resident reduced costs
 *                and handles with no_rcache.  count == 0 is valid and behaves like an empty mcf_update_costs.  Handles with
 *                shard_count > 1: MCF_E_STATE.  Nodes cannot be added: n, the root's id and the head-bucket node ranges stay.
 *   engine path  the handle keeps the path, the pricing grid (price_blocks), the sweep variant and the tree layout it was
 *                created with; the fused LDS path recomputes its LDS plan for the grown m.  Where the grown instance no longer
 *                satisfies a hard limit of that path -- the LDS capacity of the fused small-instance loop (k_solve_small) is
 *                the only one -- the call returns MCF_E_STATE with a message that names the limit, before anything changes
 *                (the way on is a new handle plus mcf_set_basis).
 *   errors       all checked before anything changes.  MCF_E_BAD_ARG: null handle, negative count, null arrays with a positive
 *                count, an end point outside [0, n), a self-loop.  MCF_E_RANGE: |cost| > INT32_MAX, big-M would reach 2^44, or
 *                m + count + n >= 2^30.  MCF_E_ALLOC: a new array cannot be allocated -- the re-layout is out of place and the
 *                pointers are swapped only after every pass has completed, so the handle is exactly as it was.  The arc arrays
 *                (and the adjacency) exist TWICE for the duration of the call.  MCF_E_HIP from a device pass AFTER the swap
 *                (the message says so) is the one failure that leaves the handle unusable: destroy it.
 *   afterwards   the static arrays -- tail / head / cost / orig / cap, the bucket offsets, the adjacency as a set per node
 *                (the order inside a node's list is not part of the contract), the priorities, the Devex granule table -- are
 *                exactly what mcf_create of the extended instance (old arcs, then the new ones in the given order) holds, and
 *                so is the host image: mcf_reset, mcf_set_basis, mcf_update_*, the certificates and the objective work on the
 *                extended instance.  Old arcs keep flow and state; new arcs have state +1 and flow 0.  parent / size / pos /
 *                order / depth / psize and the blocked list's arenas are untouched; pred words are re-indexed, the artificial
 *                arc of node v is now m' + v (in the walk records and in mcf_get_tree).  Potentials are unchanged, except below
 *                artificial tree arcs when a new cost raised big-M (the mechanism of mcf_update_costs; bigm_grew = 1).
 *                Resident reduced costs and key codes are exact for every arc where the handle keeps them: old ones carried
 *                over, not recomputed (unless big-M grew), new ones gathered from the potentials.  The solve status is back to
 *                "running" and the counters keep counting; everything derived for pricing starts over exactly as after
 *                mcf_update_costs; captured graphs are dropped; scratch of the other passes whose size depends on m is
 *                released and allocated again on its next use. */
typedef struct mcf_arcs_report {
    int64_t first_index;   /* caller's index of the first new arc = m before the call; new arc i is first_index + i */
    int64_t m;             /* arcs after the call */
    int64_t eligible;      /* new arcs with reduced cost < 0 under the resident potentials (census on the device) */
    int64_t bigm_grew;     /* 1 = a new cost raised big-M (potentials below artificial tree arcs moved, as in mcf_update_costs) */
    int64_t shifted_only;  /* old arcs that moved by a constant offset inside a chunk that received no new arc (diagnostic) */
    double  device_ms;     /* HIP events round the device passes: the stream work of the re-layout plus that of the passes after
                              the swap; the host image's own merge and the frees are outside both pairs of events */
} mcf_arcs_report;

int mcf_add_arcs(mcf_handle* h, int64_t count, const int32_t* tail, const int32_t* head, const int64_t* cost,
                 const int64_t* cap, const int8_t* arc_priority /* key_mode 2; may be NULL = 0 */,
                 mcf_arcs_report* out /* may be NULL */);

/* ---- fork a resident handle on the device.  Every edit above consumes the state it starts from; the reference's what-if
 * loops (examples/sensitivity_analysis_example.py, scenarios 1-3 and 5 of examples/incremental_resolving_example.py) go back
 * to the same optimum again and again, which on a handle meant a new mcf_create, a full upload and mcf_set_basis' host walk
 * per what-if.  mcf_fork makes `count` new handles, each a complete copy of src's resident state: every introspection call
 * (mcf_get_result with all integer fields of mcf_stats, mcf_get_tree, mcf_get_reduced_costs, mcf_get_pricing_keys,
 * mcf_get_weights, mcf_certify, mcf_cost_ranges) answers for a fork what it answers for src, bit for bit (measured times
 * aside), and any later sequence of calls makes the same pivots in the same order on a fork as on src -- in every state of
 * the handle between two solves: fresh, at an iteration limit (mid-solve), optimal, infeasible, unbounded; on every engine
 * path, tree layout, rule and key_mode; after mcf_update_* and mcf_add_arcs; with dropped reduced costs.
 *
 *   what is copied    the control block (status, counters, Devex block cursor, swap count, tuner counts, minor-iteration
 *                     state, blocked-list arena and allocation cursor), weights and touched-weight list, candidate list and
 *                     candidate cache, dirty marks, per-workgroup swept counts, both arenas of the blocked list with block
 *                     records and extents, the coarse index, reduced costs and key codes (or their absence: rc_dropped_at),
 *                     the run-shape state, arc priorities, and the host image with every host-side field a later call reads.
 *                     All device arrays of all `count` handles are written by ONE kernel launch over a segment table.
 *   what is not       scratch every pivot writes before it reads; captured graphs (rebuilt on first use); scratch of the
 *                     post-solve passes (allocated on first use).  mcf_options.arc_priority of a fork is NULL.  Decisions
 *                     mcf_create took from environment variables are inherited from src, not read again.
 *   independence      no device memory, pinned slot, stream of its own, graph or event is shared: destroying src leaves the
 *                     forks whole and the other way round.  Streams follow mcf_create's rule (pooled for small handles).
 *   src               is only read, exactly as by mcf_certify (its stream is synchronised first): a later mcf_solve of src
 *                     makes the same pivots.  A handle driven through mcf_enqueue_* must be quiescent (the caller's part).
 *
 * Errors, all before any device work: MCF_E_BAD_ARG (null src / out, count < 0), MCF_E_STATE (shard_count > 1);
 * count == 0 is MCF_OK and does nothing.  MCF_E_ALLOC / MCF_E_HIP part-way: every handle made by the call is destroyed,
 * out[0..count) is all NULL, src is untouched; the message through mcf_last_error(NULL), as for mcf_create.
 *
 * mcf_restore runs the same copy into handles that already exist, without allocating: each dst[i] must have src's shape --
 * n, m, padded m, device, rule, key_mode, engine path, tree layout geometry, pricing grid, and which of reduced costs, key
 * codes, dirty marks, candidate cache and priorities it was created with (mcf_add_arcs keeps the record current) --
 * otherwise MCF_E_STATE names the field (mcf_last_error(src)) before anything changes.  dst[i] == src, a duplicate or a
 * NULL entry: MCF_E_BAD_ARG.  Afterwards dst[i] is what a fresh fork of src would be, host image and options included;
 * its captured graphs are dropped. */
typedef struct mcf_fork_report {
    int64_t count;           /* handles written */
    int64_t segments;        /* device arrays copied per handle */
    int64_t bytes_per_fork;  /* device bytes copied per handle */
    double  device_ms;       /* HIP events round the copy launch(es) */
} mcf_fork_report;

int mcf_fork(mcf_handle* src, int32_t count, mcf_handle** out, mcf_fork_report* report /* may be NULL */);
int mcf_restore(mcf_handle* const* dst, int32_t count, mcf_handle* src, mcf_fork_report* report /* may be NULL */);

/* ---- certificate on the device (the reference's validate_flow / compute_bottleneck_arcs, utils.py:169-312, plus the dual
 * half the reference never checks).  Conservation, bounds, complementary slackness, the exact objectives and the
 * consistency of the resident basis are evaluated where the data is: one streaming pass over the arcs, one pass over the
 * nodes (conservation is a gather over the node -> arc adjacency), a final reduction; a few hundred bytes come back.
 *
 *   flow, potential   NULL = the handle's resident arrays (nothing is downloaded).  Non-NULL = the caller's arrays --
 *                     flow[m] in the caller's arc order, potential[n] with the root excluded, the layout of mcf_get_result
 *                     -- certified against the handle's instance (costs, capacities, supplies, topology).  They are
 *                     uploaded to scratch buffers; the handle's own state is not touched.  A caller's flow says nothing
 *                     about artificial arcs: node balances are then reported as they stand (validate_flow's meaning) and
 *                     artificial_flow is 0.  Caller's potentials must satisfy |potential| <= 2^61 (MCF_E_RANGE).
 *   checks            MCF_CERT_* groups, 0 = all.  BASIS and PRICING describe the resident state and are evaluated only
 *                     when flow and potential are both NULL; `checks` in the result names the groups that were evaluated.
 *   read-only         nothing the solver reads is written: status, counters, candidate lists, dirty marks, Devex weights
 *                     and tuner stay bit-identical and a later mcf_solve makes the same pivots.  Valid between solves in
 *                     any state of the handle, on every engine path, tree layout, rule and key_mode, on handles that
 *                     dropped their resident reduced costs, and on handles with shard_count > 1 (every arc is checked from
 *                     the replicated state; resident reduced costs / key codes only where the shard keeps them).
 *   arithmetic        exact integers.  rc = cost + pi[tail] - pi[head].  Sums are 128-bit (two 64-bit halves, high first,
 *                     like mcf_get_result's objective).  Every "worst" is a magnitude > 0 with the caller's index of the
 *                     FIRST arc / node attaining it (ties: lowest index; -1: none), so results compare with numpy.
 *   dual objective    of the big-M problem  min c x + bigM a  s.t.  outflow - inflow = supply, 0 <= x <= cap.  With the
 *                     sign convention of rc above, c x = -sum_v pi[v] supply[v] + sum_e rc[e] x[e], hence
 *                         dual = -sum_v pi[v] * supply[v] + sum over capped arcs with rc < 0 of rc * cap
 *                     (an uncapacitated arc with rc < 0 makes the dual infeasible: it is counted in dual_lower_count and
 *                     contributes nothing).  gap = primal + bigm_term - dual; 0 at an optimal basis.
 *   verdict           what the evidence proves, all groups 1..8 evaluated: MCF_CERT_OPTIMAL = every primal and dual count
 *                     is 0, gap is 0, no artificial flow; MCF_CERT_INFEASIBLE = the same with artificial flow > 0 (the
 *                     flow is optimal for the big-M problem over the arcs the basis still holds); else MCF_CERT_NOT_PROVEN.
 *                     An unbounded status is proven by its ray, mcf_certify_ray below (this call keeps answering
 *                     MCF_CERT_NOT_PROVEN for it); an infeasible one is proven for the CALLER'S instance by mcf_certify_cut.
 *                     proves_status = 1 when the handle's status is optimal / infeasible and the verdict says the same.
 *   errors            MCF_E_BAD_ARG: null handle, null out, unknown bits in checks.  MCF_E_NO_DEVICE as elsewhere.
 * Scratch (partials, uploads, supplies: 8 B per node, an adjacency where the handle holds none or a shard's only) is
 * allocated on first use and freed by mcf_destroy; mcf_create costs what it did. */
#define MCF_CERT_BOUNDS 1u
#define MCF_CERT_CONSERVATION 2u
#define MCF_CERT_DUAL 4u
#define MCF_CERT_OBJECTIVES 8u
#define MCF_CERT_BASIS 16u
#define MCF_CERT_PRICING 32u
#define MCF_CERT_NOT_PROVEN 0
#define MCF_CERT_OPTIMAL 1
#define MCF_CERT_INFEASIBLE 2

typedef struct mcf_certificate {
    int64_t checks;                /* groups evaluated */
    int64_t status;                /* MCF_ST_* as mcf_get_result would report it, -1 while the handle is "running" */
    int64_t verdict;               /* MCF_CERT_* */
    int64_t proves_status;
    /* primal: bounds */
    int64_t negative_flow_count, over_capacity_count, bounds_worst, bounds_worst_arc;
    /* primal: conservation (|balance| saturates at INT64_MAX) */
    int64_t imbalance_count, imbalance_worst, imbalance_worst_node;
    /* dual feasibility / complementary slackness */
    int64_t dual_lower_count, dual_lower_worst, dual_lower_arc;   /* rc < 0, flow below capacity or uncapacitated */
    int64_t dual_upper_count, dual_upper_worst, dual_upper_arc;   /* rc > 0, flow > 0 */
    /* objectives, {high, low} */
    int64_t primal[2], bigm_term[2], dual[2], gap[2];
    int64_t artificial_flow, big_m;
    /* basis consistency (resident state) */
    int64_t basic_arcs;            /* arcs marked basic + artificial tree arcs; must be n */
    int64_t basic_count_mismatch;  /* basic_arcs != n */
    int64_t tree_rc_count;         /* tree arcs with rc != 0 */
    int64_t state_flow_count;      /* state +1 with flow != 0, state -1 with flow != cap */
    int64_t tree_shape_count;      /* nodes whose parent / pos / size / depth / psize / pred-arc records disagree */
    int64_t strong_count;          /* basic arcs on a bound pointing the wrong way (what mcf_set_basis repairs) */
    /* resident pricing data */
    int64_t rc_compared, rc_mismatch_count, key_compared, key_mismatch_count;
    int64_t saturated_arcs;        /* capped arcs with flow == cap > 0 (mcf_bottlenecks at 1/1) */
    double arc_pass_ms, node_pass_ms;   /* kernel durations by HIP events */
} mcf_certificate;

int mcf_certify(mcf_handle* h, const int64_t* flow, const int64_t* potential, uint32_t checks, mcf_certificate* out);

/* compute_bottleneck_arcs (utils.py:250-312) as an exact test: the capped arcs that carry flow with
 * flow * den >= cap * num (128-bit products; num >= 0, den > 0), flow = the caller's (caller's order) or NULL = resident.
 * *count <- how many there are; idx_out[0 .. min(count, idx_cap)) <- their caller's indices in ascending order, compacted
 * on the device (idx_out may be NULL with idx_cap 0).  Read-only like mcf_certify. */
int mcf_bottlenecks(mcf_handle* h, const int64_t* flow, int64_t num, int64_t den, int64_t* idx_out, int64_t idx_cap, int64_t* count);

/* ---- witnesses of the other two verdicts, evaluated on the device.  Both calls are read-only exactly as mcf_certify is
 * (nothing the solver reads is written; a later mcf_solve makes the same pivots) and valid where it is valid: between solves
 * in any state of the handle, on every engine path (fused LDS loop, persistent mid loop, graphs, handles solved by
 * mcf_solve_batch), both tree layouts, every rule and key_mode, handles that dropped their resident reduced costs, and
 * handles with shard_count > 1 (the state is replicated).  Everything is checked before any device work is queued; after an
 * error the handle is exactly as it was.  Scratch is allocated on first use and freed by mcf_destroy.
 *
 * mcf_certify_ray -- the cycle a NON-BASIC arc closes with the resident tree, classified for the push along it.
 *   arc          caller's index, or -1 = the handle's unbounded arc (mcf_stats.unbounded_arc; MCF_E_STATE when the status is
 *                not MCF_ST_UNBOUNDED).  A basic arc or an index outside [0, m): MCF_E_BAD_ARG, as are a null handle, a
 *                null out, idx_cap < 0 and a null idx_out with idx_cap > 0.
 *   direction    from the arc's state: at its lower bound it is pushed forward (tail -> head); at capacity it is pushed
 *                backward, entering_backward = 1, and it can then never be a ray.  With t / hd the end point the push
 *                leaves from / arrives at (tail / head forward, head / tail backward) the push runs
 *                hd -> ... -> join -> ... -> t and closes through the arc.
 *   membership   node u is an ancestor-or-self of x iff pos[u] <= pos[x] < pos[u] + size[u] (logical preorder positions,
 *                dense array and blocked list alike), and u's tree arc is on the cycle iff that holds for exactly one of
 *                t and hd: one lane per node, one pass over the node records, no pointer is chased.  The join is the
 *                deepest node for which it holds for both.
 *   per arc      sense of traversal against the arc's own direction, artificial or not, capped or not, its signed cost
 *                (-cost against the direction; an artificial arc costs big-M) and its residual in the push direction
 *                (cap - flow forward, flow backward, 2^60 when there is none).
 *   idx_out      idx_out[0 .. min(length, idx_cap)) <- the cycle in push order: the arc itself, the tree arcs from hd up
 *                to the join, those from the join down to t (caller's indices; m + v for the artificial arc of node v,
 *                as in mcf_get_tree).  May be NULL with idx_cap 0. */
typedef struct mcf_ray {
    int64_t arc;               /* caller's index of the arc examined */
    int64_t entering_backward; /* 1 = the arc sits at its capacity and is pushed against its direction */
    int64_t length;            /* arcs on the cycle, `arc` included */
    int64_t join;              /* the node where the two tree paths meet */
    int64_t backward_count;    /* TREE arcs traversed against their direction */
    int64_t capped_count;      /* arcs of the cycle (`arc` included) that have a capacity */
    int64_t artificial_count;  /* artificial arcs on the cycle */
    int64_t cost;              /* signed sum of the costs round the cycle: fewer than 2^30 arcs below 2^44 each */
    int64_t reduced_cost;      /* cost[arc] + pi[tail] - pi[head] from the resident potentials, negated when entering_backward: the
                                  reduced cost in the push direction (mcf_stats.unbounded_rc).  Equals `cost` whenever every tree arc
                                  has reduced cost 0 (mcf_certificate.tree_rc_count == 0) */
    int64_t theta;             /* smallest residual on the cycle, 2^60 = no bound */
    int64_t theta_arc;         /* first arc attaining it (ties: lowest index, artificial arcs as m + v), -1 = none */
    int64_t proven;            /* 1 iff entering_backward, backward_count, capped_count and artificial_count are all 0 and cost < 0:
                                  a directed cycle of real, uncapacitated arcs of negative cost in the caller's instance, which any
                                  feasible flow can be pushed along for ever */
    double device_ms;          /* HIP events round the device passes */
} mcf_ray;

int mcf_certify_ray(mcf_handle* h, int64_t arc /* caller's index; -1 = the handle's unbounded arc */,
                    int64_t* idx_out, int64_t idx_cap, mcf_ray* out);

/* mcf_certify_cut -- a node set S whose net supply exceeds what the arcs leaving it can carry (Gale's condition): the
 * textbook witness of infeasibility, checkable from tail / head / cap / supply alone, whatever the solver did.
 *   in_S == NULL   S is computed from the resident flow: the real nodes reachable in the RESIDUAL GRAPH OF THE REAL ARCS
 *                  from the seeds.  A seed is a node whose artificial arc v -> root carries flow; arc (a, b) extends S from
 *                  a to b while flow < cap or it is uncapacitated, from b to a while flow > 0; artificial arcs are never
 *                  traversed.  S is the least fixpoint and depends on no launch geometry or visiting order.  It is built
 *                  level by level over the node -> arc adjacency (the handle's, or the certificate's own, built on first
 *                  use): every adjacency list is expanded once, marks are idempotent stores, the rounds are queued on the
 *                  engine's stream in batches of 32 with one look at the "deepest level" word per batch, and the loop is
 *                  bounded by n rounds in code.
 *   in_S != NULL   the caller's set (in_S[v] != 0: v is in S).  No search is run and no flow is read: valid in any state of
 *                  the handle, a fresh one included -- a cut is a property of the instance alone.  seeds, rounds,
 *                  deficit_in_S, leaving_unsaturated, entering_with_flow and artificial_out are then 0.
 *   evaluation     one streaming pass over the arcs in engine order (bucketed by head, non-temporal loads from 4 M arcs
 *                  on, as in mcf_certify), one pass over the nodes, 128-bit sums merged in any order.
 *   S_out          S_out[v] <- 1 / 0 for every real node (may be NULL); one byte per node crosses the bus.
 *   why it works   at an "infeasible" verdict that mcf_certify attests, the computed S holds no node whose artificial arc
 *                  root -> v carries flow: a residual path from a seed to such a node would close, through the two artificial
 *                  arcs -- both still basic, since they carry flow --, a cycle of cost (path) - 2 big-M < 0, which the
 *                  optimality of the big-M problem excludes.  No leaving arc has room and no entering arc carries flow (S is
 *                  closed), so conservation over S reads supply(S) - capacity(leaving) = artificial_out: excess ==
 *                  artificial_out > 0, and the capacities are finite.  A handle without seeds (optimal, fresh) has an empty S
 *                  and proven = 0: MCF_OK, not an error.  A mid-solve handle may show deficit_in_S > 0 or leaving arcs with
 *                  room: what is there is reported.
 *   errors         MCF_E_BAD_ARG: null handle, null out. */
typedef struct mcf_cut {
    int64_t seeds;                  /* nodes of S whose artificial arc v -> root carries flow */
    int64_t nodes_in_S;
    int64_t rounds;                 /* levels of the search (rounds that found a frontier to expand) */
    int64_t deficit_in_S;           /* nodes of S whose artificial arc root -> v carries flow */
    int64_t leaving_arcs;           /* arcs with their tail in S and their head outside */
    int64_t leaving_uncapacitated;
    int64_t leaving_unsaturated;    /* leaving arcs with room under the resident flow (uncapacitated, or flow < cap) */
    int64_t entering_with_flow;     /* arcs into S that carry resident flow */
    int64_t capacity[2];            /* {high, low}: sum of the capacities of the capped leaving arcs */
    int64_t supply[2];              /* sum of the supplies over S */
    int64_t excess[2];              /* supply - capacity */
    int64_t artificial_out[2];      /* artificial flow S -> root minus root -> S (resident flow).  NOT mcf_stats.artificial_flow: that
                                       adds up the artificial arcs of both senses, and what goes to the root equals what comes from
                                       it, so at an attested "infeasible" verdict artificial_flow == 2 * artificial_out == 2 * excess */
    int64_t proven;                 /* 1 iff leaving_uncapacitated == 0 and excess > 0 */
    double device_ms;               /* HIP events round the device passes (search and evaluation) */
} mcf_cut;

int mcf_certify_cut(mcf_handle* h, const int8_t* in_S /* [n] caller's set, or NULL = compute from the resident flow */,
                    int8_t* S_out /* [n] or NULL */, mcf_cut* out);

/* ---- cost ranging on the resident basis: how far may ONE arc's cost move before the basis the handle holds stops being
 * optimal?  The question before a mcf_update_costs: an edit inside the range re-solves in zero pivots.  Answered for all arcs
 * at once, on the device, from the arrays that are already there; nothing is tried and nothing is changed.
 *
 *   definition   exact signed integers.  rc[f] = cost[f] + pi[tail f] - pi[head f] is gathered from the resident potentials on
 *                every call (the resident reduced-cost copies and key codes are not read, so handles that dropped them,
 *                no_rcache handles and shards answer alike).  The slack of a NON-BASIC arc is s[f] = state[f] * rc[f]; the
 *                engine prices f in exactly when s[f] < 0.
 *                  non-basic at its lower bound (state +1):  down = s,  up = MCF_RANGE_INF
 *                  non-basic at its capacity    (state -1):  down = MCF_RANGE_INF,  up = s
 *                  basic arc e with child end v, S = the subtree of v: over the non-basic real arcs with exactly one end in S
 *                      P[v] = min( s[f] : tail f in S, state -1 ;  s[f] : head f in S, state +1 )
 *                      N[v] = min( s[f] : tail f in S, state +1 ;  s[f] : head f in S, state -1 )
 *                    (an empty set gives MCF_RANGE_INF), and  up = N, down = P  when v is the tail of e,  up = P, down = N
 *                    when v is its head: raising cost[e] by d moves the potentials of S by -d / +d, an arc with its tail in S
 *                    sees rc + that shift, one with its head in S rc - it.
 *                Artificial arcs have no range: those that left the basis are never priced and constrain nothing, those in
 *                the tree have no caller's cost (they still lie on other arcs' paths).
 *   contract     on an optimal handle, any single change cost[e] -> c with cost[e] - down[e] <= c <= cost[e] + up[e] leaves no
 *                eligible arc: mcf_solve makes 0 pivots.  One unit past a finite end makes the arc(s) that attain it eligible,
 *                with violation 1.  RANGES ARE STATED AT FIXED BIG-M: a new cost that makes mcf_update_costs raise
 *                big-M (|c| + 1) * (n + 2) > big_m moves the potentials below artificial tree arcs as well, which this call
 *                does not follow; report.big_m is the value the answer holds for.  The numeric domain |cost| <= INT32_MAX is
 *                a separate limit and is not folded in either: an end may lie outside it.
 *   negative     slacks are not clamped.  On a basis that is not optimal (mid-solve, after an edit, a planted basis) a
 *                negative entry comes through as it is and means "this side of the range is already empty": the arc, or an
 *                arc across its cut, prices in as things stand.  report.eligible counts the non-basic arcs with s < 0.
 *   arc, count   caller's indices, duplicates allowed, down[i] / up[i] answer arc[i]; count < 0 with arc == NULL = all m arcs
 *                in the caller's order.  With a list only `count` entries cross the bus.
 *   method       binary lifting over parent pointers, O((n + m) log depth) whatever the shape of the tree and the same on
 *                both tree layouts: the greatest depth is reduced first (one word comes back: K = max(1, bit_length) levels),
 *                ancestor tables anc[k][v] are built level by level, every non-basic arc lowers one table cell per jump of its
 *                two tree paths (64-bit atomic min, skipped where the cell is already low enough), and the levels are pushed
 *                down into one value per tree arc.  Integer mins only: no launch geometry or merge order changes a bit.
 *   read-only    exactly as mcf_certify: nothing the solver reads is written and a later mcf_solve makes the same pivots.
 *                Valid between solves in any state of the handle, on every engine path, both tree layouts, every rule and
 *                key_mode, handles that dropped their resident reduced costs, and handles with shard_count > 1 (the state is
 *                replicated).  m == 0 or n == 1: MCF_OK with an empty answer.
 *   errors       MCF_E_BAD_ARG, all checked before any device work: null handle; null down / up with entries to return; count
 *                > 0 with a null list or count < 0 with one; an index outside [0, m).  MCF_E_ALLOC: the tables cannot be
 *                allocated; the handle is untouched.
 * Scratch -- the tables, 20 B x K x (n + 1), the answer, 16 B x m, the list -- is allocated on first use, released and
 * allocated again when K or m outgrew it, and freed by mcf_destroy. */
#define MCF_RANGE_INF INT64_MAX
typedef struct mcf_ranges_report {
    int64_t basic_real, basic_artificial, eligible;   /* eligible == 0 <=> no arc prices in */
    int64_t max_depth, levels;                        /* greatest depth of the tree; K */
    int64_t inf_down, inf_up;                         /* entries equal to MCF_RANGE_INF among those returned */
    int64_t big_m;                                    /* the big-M the ranges are stated at */
    double  device_ms;                                /* HIP events round the device passes (the depth pass and the rest) */
} mcf_ranges_report;
int mcf_cost_ranges(mcf_handle* h, int64_t count, const int64_t* arc /* caller's indices; count < 0 and NULL = all m */,
                    int64_t* down, int64_t* up, mcf_ranges_report* out /* may be NULL */);

/* ---- flow ranging on the resident basis: how far may ONE supply shift or ONE arc's capacity move before a tree flow leaves
 * its bounds, and what does the objective do until then?  The question before a mcf_update_rhs: an edit inside the range takes
 * path 0 -- the basis stays, nothing pivots -- and costs exactly rate * d.  The primal mirror image of mcf_cost_ranges, from
 * the same resident arrays; nothing is tried and nothing is changed.
 *
 *   definition   exact signed integers, the state as mcf_certify reads it.  The tree arc of node v (pred >> 1; it points child
 *                -> parent when pred & 1) has two residuals:
 *                                   push along the arc                     push against it
 *                  capped           cap - flow                             flow
 *                  uncapacitated    MCF_RANGE_INF                          flow
 *                  artificial       MCF_RANGE_INF (the push raises         flow (past it mcf_update_rhs turns the arc round and
 *                                   artificial flow: see art_rising)       the potentials below it move by 2 big-M)
 *                U[v] is the residual for a push child -> parent, D[v] for parent -> child.  push(x -> y) = the largest amount
 *                the tree carries from x to y = min(U over the tree arcs from x up to the join, D over those from the join
 *                down to y); MCF_RANGE_INF and no arc for x == y.  limit_arc is the FIRST arc in push order (x up to the join,
 *                then the join down to y) that attains the limit, as a caller's index, m + v for the artificial arc of node v
 *                as in mcf_get_tree, -1 when the limit is MCF_RANGE_INF.  No launch geometry enters that rule.  art_rising is
 *                the number of artificial arcs on the path whose flow the push raises.  Residuals are not clamped: a state
 *                that is out of bounds reports what is there (a negative limit: the range is already empty).
 *   supply       pair i asks for the edit supply[from[i]] += d, supply[to[i]] -= d:  limit = push(from -> to),  rate =
 *                pi[to] - pi[from] = the signed cost of the tree path, the exact change of the big-M objective per unit.
 *   capacity     by how much may the capacity of one arc fall (down) or rise (up); rate = objective per unit of capacity ADDED
 *                  uncapacitated                        down INF           up INF           rate 0    no arcs
 *                  capped, non-basic at lower bound     down cap           up INF           rate 0    no arcs
 *                  capped, basic                        down cap - flow    up INF           rate 0    down_arc = the arc itself
 *                  non-basic at capacity, t -> hd       down min(push(t -> hd), cap)   up push(hd -> t)   rate rc = cost + pi[t] - pi[hd]
 *                an arc at capacity carries its capacity: more of it sends more t -> hd, which the tree returns hd -> t; less
 *                of it the other way round.  down_arc / up_arc come from the push; down_arc is the arc itself when cap is
 *                strictly the smaller of the two.
 *   contract     the handle holds a basis with wrong_way == 0 (an optimal one does), the edit is one supply shift or one
 *                capacity change of size d through mcf_update_rhs (in rate * d a capacity that FALLS by d counts as -d):
 *                  0 < d < limit    path 0 with tree_violations == 0 and art_flips == 0; on an optimal handle the next
 *                                   mcf_solve makes 0 pivots and mcf_certify gives primal + bigm_term = the old value + rate * d;
 *                  d == limit       tree_violations == 0; the path may be 1, because the arc that reached its bound can point
 *                                   the wrong way; after mcf_solve the objective is still the old value + rate * d;
 *                  d == limit + 1   tree_violations >= 1 when 0 <= limit_arc < m, art_flips >= 1 when limit_arc >= m (a capacity
 *                                   cannot fall below 0: where down == cap there is no such edit);
 *                  art_rising > 0   any d > 0 leaves artificial flow: on a handle that was optimal the edited instance is infeasible.
 *                Ranges for several edits at once, for capping an uncapacitated arc and beyond the flip of an artificial arc
 *                are not given.
 *   lists        from / to: node indices, arc: caller's arc indices; duplicates allowed, entry i answers pair / arc i; for
 *                capacities count < 0 with arc == NULL = all m arcs in the caller's order.  Every output array may be NULL.
 *   method       k_rng_depth and the ancestor tables of mcf_cost_ranges; two more tables hold min U / min D over the tree arcs
 *                of v and its next 2^k - 1 ancestors together with the attaining node (ties: the lower half upwards, the upper
 *                half downwards), built level by level; every query reads one cell per jump of its two tree paths, at most
 *                3 K + 2 jumps, and an arc at capacity asks both directions in one enumeration.  Gather only, no atomics.
 *   report       basic_real / basic_artificial: the tree arcs; at_capacity: the non-basic arcs at capacity (capacity call; 0
 *                from the supply call); inf_count / zero_count: returned sides (limit; down and up) equal to MCF_RANGE_INF / 0;
 *                art_rising_count: pairs returned with art_rising > 0 (supply call), pushes of arcs at capacity -- two per
 *                arc, all arcs of the handle -- that raise artificial flow (capacity call).
 *   read-only    exactly as mcf_certify and mcf_cost_ranges: nothing the solver reads is written and a later mcf_solve makes
 *                the same pivots.  Valid between solves in any state of the handle, on every engine path, both tree layouts,
 *                every rule and key_mode, handles that dropped their reduced costs and handles with shard_count > 1.
 *                count == 0, n == 1, and for capacities m == 0: MCF_OK without device work (pairs of the one node with itself
 *                get MCF_RANGE_INF, no arc, rate 0).
 *   errors       MCF_E_BAD_ARG, all checked before any device work: null handle; a node outside [0, n) or an arc outside
 *                [0, m); null lists with count > 0; a list together with count < 0 (capacities), count < 0 (supplies).
 *                MCF_E_ALLOC: scratch cannot be allocated; the handle is untouched.
 * Scratch -- the tables of mcf_cost_ranges plus 8 B x K x (n + 1), the answers 40 B x m / 28 B x count, the lists -- is allocated
 * on first use, shared with mcf_cost_ranges where it is the same, and freed by mcf_destroy. */
typedef struct mcf_flow_ranges_report {
    int64_t basic_real, basic_artificial, at_capacity;
    int64_t max_depth, levels;                        /* greatest depth of the tree; K */
    int64_t inf_count, zero_count;                    /* returned sides equal to MCF_RANGE_INF / to 0 */
    int64_t art_rising_count;
    int64_t big_m;                                    /* the big-M the rates are stated at */
    double  device_ms;                                /* HIP events round the device passes (the depth pass and the rest; the
                                                         upload of the lists is not counted) */
} mcf_flow_ranges_report;
int mcf_supply_ranges(mcf_handle* h, int64_t count, const int32_t* from, const int32_t* to,
                      int64_t* limit, int64_t* limit_arc, int64_t* rate, int32_t* art_rising /* each may be NULL */,
                      mcf_flow_ranges_report* out /* may be NULL */);
int mcf_capacity_ranges(mcf_handle* h, int64_t count, const int64_t* arc /* count < 0 and NULL = all m */,
                        int64_t* down, int64_t* up, int64_t* down_arc, int64_t* up_arc, int64_t* rate /* each may be NULL */,
                        mcf_flow_ranges_report* out /* may be NULL */);

/* ---- arc-sharded multi-GPU pivoting: one handle per rank, every rank holds the full
 * replicated state and prices only its shard (options.shard_rank / shard_count).  Per pivot:
 *   mcf_enqueue_price   local best candidate -> cand_out (device, 2 x int64: key, packed arc id)
 *   <RCCL all-gather of the 16-byte candidates, by the caller, on the same stream>
 *   mcf_enqueue_pivot   every rank applies the same winning pivot to its replica
 * `stream` is a hipStream_t (0 = default stream).  Nothing here synchronises. */
int mcf_enqueue_price(mcf_handle* h, void* stream, int64_t* cand_out_dev);
int mcf_enqueue_pivot(mcf_handle* h, void* stream, const int64_t* cands_dev, int32_t ncand);
/* Candidate-list rule over several ranks -- the amortisation lever of SURVEY.md section 8e: ONE collective per
 * (minor_cap + 1) pivots instead of one per pivot.
 *   mcf_shard_info          list_len = candidates one sweep of this handle leaves (one per pricing workgroup);
 *                           minor_cap = pivots that may re-price a list before the next sweep (simplex_pricing.py:398-400)
 *   mcf_enqueue_price_list  sweep the shard; cands_out (device, list_len x {key, packed arc id}) <- its candidates
 *   <all-gather of the lists, by the caller>
 *   mcf_enqueue_pivots      `count` pivots on the gathered list: the first takes the sweep's keys, the others re-price
 *                           the listed arcs against the current potentials (minor iterations, simplex_pricing.py:419-456)
 * With shard_count > 1 a handle patches the resident reduced costs of its own shard only (1 / shard_count of the
 * update work); listed arcs of other shards are re-priced from the replicated potentials. */
int mcf_shard_info(mcf_handle* h, int32_t* list_len, int32_t* minor_cap);
int mcf_enqueue_price_list(mcf_handle* h, void* stream, int64_t* cands_out_dev);
int mcf_enqueue_pivots(mcf_handle* h, void* stream, const int64_t* cands_dev, int32_t ncand, int32_t count);
/* Read the control block (synchronises `stream`): status (MCF_ST_* or -1 = still running). */
int mcf_poll(mcf_handle* h, void* stream, int32_t* status_or_running, int64_t* pivots);
int mcf_set_max_pivots(mcf_handle* h, int64_t max_total_pivots);

/* ---- measurement helpers (bench.py) */
/* Launch the pricing kernel `reps` times back to back on the engine stream between two HIP
 * events; *ms_per_launch = average duration.  Read-only with respect to the solver state. */
int mcf_time_pricing(mcf_handle* h, int32_t rule, int32_t reps, double* ms_per_launch);
/* Device-to-device copy of `bytes` bytes, `reps` times, between two HIP events: the measured
 * HBM copy ceiling quoted beside the datasheet peak. */
int mcf_time_copy(int32_t device, int64_t bytes, int32_t reps, double* ms_per_copy);

/* ---- introspection for the parity tests: raw tree state, host copies.
 * parent[n+1], pred_arc[n+1] (-1 for the root), size[n+1], pos[n+1], order[n+1], state[m],
 * potential_with_root[n+1], depth[n+1], psize[n+1] (subtree size of the node at each preorder
 * position).  Any pointer may be NULL. */
int mcf_get_tree(mcf_handle* h, int32_t* parent, int32_t* pred_arc, int32_t* size, int32_t* pos,
                 int32_t* order, int8_t* state, int64_t* potential_with_root, int32_t* depth, int32_t* psize);

/* Reduced cost of every arc (caller's order) as the pricing kernel sees it: the resident copy
 * when the handle keeps one (*resident = 1), else cost + pi[tail] - pi[head] computed on the host.
 * Tests use it to check the invariant resident rc == cost + pi[tail] - pi[head]. */
int mcf_get_reduced_costs(mcf_handle* h, int64_t* rc_out, int32_t* resident);

/* The compressed Dantzig key of every arc (caller's order) as the sweep reads it; *present = 0 (and zeros) when the
 * handle keeps none.  Tests check the invariant key == code(-state * reduced cost) and decode it with the documented
 * scheme (csrc/mcf_core.h: mcf_vkey). */
int mcf_get_pricing_keys(mcf_handle* h, int32_t* keys_out, int32_t* present);

/* Devex reference weights of every arc (caller's order; 1.0 for a handle that never priced with the Devex rule).
 * With mcf_get_tree / mcf_get_result this is the full input of one block selection, so that a test can replay
 * mcf_price_once(MCF_RULE_DEVEX_BLOCK, ...) on the oracle's restated _select_entering_arc_vectorized. */
int mcf_get_weights(mcf_handle* h, float* weight_out);

/* ---- native DIMACS "p min" reader (host only; replaces benchmarks/parsers/dimacs.py:105-286 for
 * instances too large for one Python object per arc).  Two calls: mcf_dimacs_scan returns the
 * counts, mcf_dimacs_load fills caller-allocated arrays (0-based node ids; cap -1 = uncapacitated,
 * also for the reference's "-1" / "inf" / >= 1e15 conventions, dimacs.py:216-221; 4-field arc lines
 * mean lower = 0, dimacs.py:202-207).  Integer data only: a non-integral token is an error.
 * Return 0 or MCF_E_BAD_ARG with a message in err (may be NULL). */
int mcf_dimacs_scan(const char* path, int64_t* n_nodes, int64_t* n_arcs, char* err, int32_t err_len);
int mcf_dimacs_load(const char* path, int64_t n_nodes, int64_t n_arcs, int32_t* tail, int32_t* head,
                    int64_t* lower, int64_t* cap, int64_t* cost, int64_t* supply, char* err, int32_t err_len);

const char* mcf_last_error(mcf_handle* h); /* NULL handle: last create-time error of this thread */
void mcf_destroy(mcf_handle* h);
int mcf_abi_version(void);
/* Number of usable HIP devices (0 when none); never initialises a context. */
int mcf_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MCF_H */
