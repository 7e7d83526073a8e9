"""Inputs of the pricing-rule tests (``test_rule_reference_cpu.py``, ``test_gpu_rule_reference.py``).  A plain helper like
``small_loop_instances.py``: seeded, no fixtures, every result computed once and never changed.  Every instance fits the fused
LDS loop (at most 3 072 arcs, at most 256 nodes) and exists to reach ONE event of the rule state of ``rule_reference.py`` from a
cold start; ``test_rule_reference_cpu.py`` asserts that the reference's trajectory really contains it.

* ``flips_1100``: two hubs joined by a tree path of ample capacity, and 1 100 parallel arcs of capacity 1 between them that are all
  cheaper than the path: each enters and leaves at once (a bound flip).  More than 1 024 pivots with fewer than 64 basis swaps: the
  touched-weight list is full after pivot 1 024 and pivot 1 025 is the early reset; every pivot counts as degenerate for the tuner,
  which grows the block to its cap of 64 granules and stops there (from 8 granules, m >= 1 000: 8, 12, 18, 27, 40, 60, 64; with the
  block size asked for as m / 4 and the tuner switched on: 16, 24, 36, 54, 64; with m / 8 asked for the tuner is off and the
  blocks stay at 8 granules: only there the early reset's return to block 0 changes the next entering arc);
* ``swaps_200``: netgen-style, at least 200 basis swaps -- three resets -- with a bound flip among the first 64 swaps;
* ``shrink_to_1``: a transportation instance of generic supplies and no capacities: hardly a degenerate pivot, so the tuner
  shrinks the block 16, 12, 9, 6, 4, 3, 2, 1;
* ``empty_blocks``: netgen-style, run with blocks of ONE granule and the tuner off: 64 blocks, of which ever fewer hold an
  eligible arc, so that the search walks 63 empty blocks to the last one that does, and 64 for the verdict;
* ``stay_vs_cyclic``: netgen-style; staying on a block and advancing after every pivot part ways within 20 pivots;
* ``direction_ties``: few different costs, small capacities: a forward and a backward arc share the largest merit of a block,
  where the backward one has to win;
* ``list_periods``: for the candidate list: 3 000 arcs of which half end in the first head bucket, so that 8, 16 and 64 pricing
  workgroups make lists of different arcs (the bucket's second and third run of 1 024 arcs go to further workgroups);
* ``devex_nodes_128`` / ``devex_nodes_129``: netgen-style with 128 and 129 tree nodes (the root included): under Devex the fused
  loop runs 256 lanes wide up to 128 tree nodes and 1 024 wide beyond."""

from __future__ import annotations

import functools

import numpy as np

import planted_pivots as pp
import rule_reference as rr
from network_flow_solver_amd import generators
from network_flow_solver_amd.generators import ArcSoA

FLIP_ARCS = 1100
FLIP_PATH = 9                     # tree arcs between the hubs


@functools.lru_cache(maxsize=None)
def flips_1100() -> ArcSoA:
    n = FLIP_PATH + 1                                           # hub 0, the path's inner nodes, hub n - 1
    rng = np.random.default_rng([1100, 1])
    path_t, path_h = np.arange(n - 1), np.arange(1, n)
    m = FLIP_ARCS + FLIP_PATH
    tail, head = np.zeros(m, np.int64), np.full(m, n - 1, np.int64)
    cost, cap = rng.integers(1, 51, m), np.ones(m, np.int64)    # parallel arcs: cheaper than the path's 9 x 10, many equal costs
    at = np.sort(rng.choice(m, FLIP_PATH, replace=False))       # the path's arcs strewn among them
    tail[at], head[at], cost[at], cap[at] = path_t, path_h, 10, -1
    supply = np.zeros(n, np.int64)
    supply[0], supply[n - 1] = 5000, -5000
    return ArcSoA(n, tail.astype(np.int32), head.astype(np.int32), cost.astype(np.int64), cap, supply, "flips_1100")


@functools.lru_cache(maxsize=None)
def swaps_200() -> ArcSoA:
    return generators.netgen_style(96, 640, seed=3, name="swaps_200")


@functools.lru_cache(maxsize=None)
def shrink_to_1() -> ArcSoA:
    """100 sources (nodes 0 .. 99), 100 sinks, 990 arcs without capacities; arc i < 100 joins source i and sink i, the others are
    random.  Supplies and demands are what a random flow on 300 of the arcs needs: feasible, and generic."""
    ns, nt, m = 100, 100, 990
    rng = np.random.default_rng([400, 8])
    tail = np.concatenate((np.arange(ns), rng.integers(0, ns, m - ns)))
    head = ns + np.concatenate((np.arange(nt), rng.integers(0, nt, m - nt)))
    ships = np.zeros(m, np.int64)
    ships[:ns] = rng.integers(1000, 100000, ns)
    some = ns + rng.choice(m - ns, 200, replace=False)
    ships[some] = rng.integers(1000, 100000, 200)
    supply = np.zeros(ns + nt, np.int64)
    np.add.at(supply, tail, ships)
    np.subtract.at(supply, head, ships)
    return ArcSoA(ns + nt, tail.astype(np.int32), head.astype(np.int32), rng.integers(1, 1001, m).astype(np.int64), np.full(m, -1, np.int64),
                  supply, "shrink_to_1")


@functools.lru_cache(maxsize=None)
def empty_blocks() -> ArcSoA:
    return generators.netgen_style(64, 512, seed=1, name="empty_blocks")


@functools.lru_cache(maxsize=None)
def stay_vs_cyclic() -> ArcSoA:
    return generators.netgen_style(100, 800, seed=4, name="stay_vs_cyclic")


@functools.lru_cache(maxsize=None)
def list_periods() -> ArcSoA:
    """netgen_style(200, 1500) plus 1 500 arcs into nodes 0 .. 24, the first head bucket, costed like the others."""
    base = generators.netgen_style(200, 1500, seed=6)
    extra = 1500
    rng = np.random.default_rng([3000, 6])
    head = rng.integers(0, 25, extra)
    tail = rng.integers(25, 200, extra)
    cost = rng.integers(int(base.cost.min()), int(base.cost.max()) + 1, extra)
    cap = rng.integers(1, max(int(base.cap[base.cap > 0].max()), 2) + 1, extra)
    return ArcSoA(base.n, np.concatenate((base.tail, tail)).astype(np.int32), np.concatenate((base.head, head)).astype(np.int32),
                  np.concatenate((base.cost, cost)).astype(np.int64), np.concatenate((base.cap, cap)).astype(np.int64), base.supply.copy(),
                  "list_periods")


@functools.lru_cache(maxsize=None)
def direction_ties() -> ArcSoA:
    """24 nodes on a ring of ample capacity and cost 8, 176 random arcs of costs 1 .. 4 and capacities 1 .. 3: with so few
    different costs and so many arcs that fill up, a forward and a backward arc often share the largest merit of a block."""
    n, m = 24, 200
    rng = np.random.default_rng([77, n, m, 1])
    t = rng.integers(0, n, m)
    h = (t + 1 + rng.integers(0, n - 1, m)) % n
    t[:n], h[:n] = np.arange(n), (np.arange(n) + 1) % n
    cost, cap = rng.integers(1, 5, m), rng.integers(1, 4, m)
    cap[:n], cost[:n] = -1, 8
    supply, k = np.zeros(n, np.int64), n // 4
    ends = rng.choice(n, 2 * k, replace=False)
    supply[ends[:k]] = rng.integers(1, 6, k)
    supply[ends[k:]] = 0
    supply[ends[k:]] = -rng.multinomial(int(supply.sum()), np.ones(k) / k)
    return ArcSoA(n, t.astype(np.int32), h.astype(np.int32), cost.astype(np.int64), cap.astype(np.int64), supply, "direction_ties")


@functools.lru_cache(maxsize=None)
def devex_nodes(tree_nodes: int) -> ArcSoA:
    return generators.netgen_style(tree_nodes - 1, 4 * tree_nodes, seed=5, name=f"devex_nodes_{tree_nodes}")


INSTANCES = {"flips_1100": flips_1100, "swaps_200": swaps_200, "shrink_to_1": shrink_to_1, "empty_blocks": empty_blocks,
             "stay_vs_cyclic": stay_vs_cyclic, "direction_ties": direction_ties, "list_periods": list_periods, "devex_nodes_128": lambda: devex_nodes(128),
             "devex_nodes_129": lambda: devex_nodes(129)}

# (case id, instance, rule, options of the reference = options of the engine)
DEVEX, LIST = 1, 2
CASES = {
    "flips_1100": ("flips_1100", DEVEX, {}),
    "flips_1100_quarter": ("flips_1100", DEVEX, dict(block_size=(FLIP_ARCS + FLIP_PATH) // 4, tuner=1)),
    # blocks of 8 granules that stay: the early reset's return to block 0 shows in the very next entering arc
    "flips_1100_fixed": ("flips_1100", DEVEX, dict(block_size=(FLIP_ARCS + FLIP_PATH) // 8, tuner=-1)),
    "swaps_200": ("swaps_200", DEVEX, {}),
    "swaps_200_stay": ("swaps_200", DEVEX, dict(stay=True)),
    "swaps_200_fixed": ("swaps_200", DEVEX, dict(block_size=100)),            # a caller's block size: the tuner is off
    "shrink_to_1": ("shrink_to_1", DEVEX, {}),
    "empty_blocks": ("empty_blocks", DEVEX, dict(block_size=8, tuner=-1)),
    "empty_blocks_stay": ("empty_blocks", DEVEX, dict(block_size=8, tuner=-1, stay=True)),
    "stay_vs_cyclic": ("stay_vs_cyclic", DEVEX, {}),
    "stay_vs_cyclic_stay": ("stay_vs_cyclic", DEVEX, dict(stay=True)),
    "direction_ties": ("direction_ties", DEVEX, {}),
    "direction_ties_stay": ("direction_ties", DEVEX, dict(stay=True)),
    "devex_nodes_128": ("devex_nodes_128", DEVEX, {}),
    "devex_nodes_129": ("devex_nodes_129", DEVEX, {}),
    "list_periods_8": ("list_periods", LIST, dict(price_blocks=8)),
    "list_periods_16": ("list_periods", LIST, dict(price_blocks=16)),
    "list_periods_64": ("list_periods", LIST, dict(price_blocks=64)),
    "swaps_200_list": ("swaps_200", LIST, dict(price_blocks=8)),
}
STATE_KEYS = ("flow", "state", "potential", "parent", "pred_arc", "depth", "size")
WINDOW = 2                        # pivots compared one by one before and after every event
FIRST = pp.K_PIVOTS


def instance(name: str) -> ArcSoA:
    return INSTANCES[name]()


def new_reference(cid: str):
    name, rule, opt = CASES[cid]
    cls = rr.DevexRef if rule == DEVEX else rr.CandidateListRef
    return cls(pp.cold_plant(instance(name)), **opt)


def _counters(ref) -> dict:
    d = dict(pivots=ref.pivots, degenerate=int(ref.degenerate_count), bound_flips=int(ref.flips), arcs_priced=ref.arcs_priced)
    if isinstance(ref, rr.CandidateListRef):
        d.update(minor_pivots=ref.minor_pivots, major_sweeps=ref.major_sweeps)
    else:
        d.update(block_index=ref.block_index, block_granules=ref.block_granules)
    return d


def _chosen_period_ends(ref):
    """Of a candidate list's period ends, the ones a GPU run halts at: the first two, the first period that used all its minor
    pivots, the first whose list emptied early (and had taken a minor pivot, where there is one), and the last two."""
    ends = [e for e in ref.events if e[1] == "period_end"]
    assert len(ends) == len(ref.periods) or (len(ends) == len(ref.periods) - 1 and ref.periods[-1][1] == "open")
    pick = {0, 1, len(ends) - 2, len(ends) - 1}
    kinds = [p[1] for p in ref.periods[:len(ends)]]
    pick.add(kinds.index("full") if "full" in kinds else 0)
    emptied = [i for i, p in enumerate(ref.periods[:len(ends)]) if p[1] == "emptied"]
    taken = [i for i in emptied if ref.periods[i][0] > 0]
    pick.update((taken or emptied or [0])[:1])
    return [ends[i] for i in sorted(pick) if 0 <= i < len(ends)]


@functools.lru_cache(maxsize=None)
def trajectory(cid: str) -> dict:
    """The reference's whole run on a case, computed once, shared by the tests and never changed: entering[k - 1] of pivot k
    (flip[k - 1]: it was a bound flip, degenerate[k - 1]: it moved no flow), events, stops (the pivot numbers at which a GPU run
    halts: 1 .. 6 and from 2 before to 2 after every event -- of a candidate list: every chosen period end --, the last pivot
    excluded, so that the closing solve() still makes one), snaps[k] at every stop (state, weights and counters after pivot k,
    ``reset`` = pivot k reset the weights), and the final snapshot, totals, objective and status."""
    ref = new_reference(cid)
    devex = isinstance(ref, rr.DevexRef)
    entering, flip, degenerate, every = [], [], [], {}
    while ref.step():
        entering.append(ref.entering)
        flip.append(bool(ref.flip))
        degenerate.append(bool(ref.degenerate))
        s = {k: getattr(ref, k).copy() for k in STATE_KEYS}
        s.update(_counters(ref))
        if devex:
            s.update(weights=ref.weights.copy(), reset=ref.just_reset)
        every[ref.pivots] = s
    total = ref.pivots
    events = list(ref.events)
    stops = set(range(1, FIRST + 1))
    for k, _ in (events if devex else _chosen_period_ends(ref)):
        stops.update(range(k - WINDOW, k + WINDOW + 1))
    stops = sorted(k for k in stops if 1 <= k < total)
    final = {k: getattr(ref, k).copy() for k in STATE_KEYS}
    final.update(_counters(ref))
    if devex:
        final.update(weights=ref.weights.copy())
    out = dict(entering=np.array(entering, np.int64), flip=np.array(flip), degenerate=np.array(degenerate), events=events, stops=stops,
               snaps={k: every[k] for k in stops}, final=final, total=total, objective=ref.objective(), status=ref.status)
    if devex:
        out.update(pass_log=list(ref.pass_log))
    else:
        out.update(periods=[tuple(p) for p in ref.periods], list_len=ref.list_len, minor_cap=ref.minor_cap)
    return out
