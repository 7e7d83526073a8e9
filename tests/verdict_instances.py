"""Seeded instances for every verdict of the engine -- optimal, unbounded, infeasible -- with UNCAPACITATED arcs in play,
plus the exact yardsticks the verdict tests compare against.  A plain helper like ``wide_range_instances.py``, on which it
is built (``wri.make``: |cost| up to INT32_MAX, capacities and supplies of 2^40, negative and zero costs).

Every instance has its outcome BY CONSTRUCTION, so no seed ever has to be skipped:

* ``uncapacitated``: a share of the arcs with cost >= 0 (ring arcs included) lose their bound, the encoding drawn from
  {-1, 2^60, 2^62, INT64_MAX}; a few capped arcs of cost >= 20 000 get exactly 2^60 - 1, which IS a bound.  Feasible: caps
  only grow.  Bounded: every negative arc stays capped.  Flows stay below 2^60 (the caller's obligation under "flows" in
  include/mcf.h): a basic solution decomposes into paths (the supply) and cycles through a non-basic arc at its capacity,
  so no arc carries more than the supply plus the sum of the finite capacities -- asserted < 2^60, the 2^60 - 1 bounds left
  out, which can never fill: a cycle that could fill one has only unbounded arcs besides, i.e. arcs of cost >= 0.
* ``unbounded``: the above plus a directed cycle of ``cycle_len`` uncapacitated arcs over distinct nodes, costs
  +a, -a, +b, -b, ... with a in [1, 3] and one arc 1 cheaper: mixed sign, total -1.  (Why so small: any subset of these
  arcs sums to >= -(3 cycle_len / 2 + 1) > -20 000, so even here no negative cycle passes through a 2^60 - 1 bound with
  nothing but unbounded arcs around it.)  The planted arcs are the LAST ``cycle_len`` arcs.
* ``infeasible``: ``uncapacitated`` with the largest sink starved / isolated, or a cut of too little capacity.
* ``deep_unbounded``: a chain whose verdict pivot closes a cycle of n - 1 arcs.

Yardsticks on Python ints only: ``unbounded_certificate`` (walks the tree; no other solver), ``infeasibility_truth``
(networkx on the big-M extension), ``wri.exact_certificate`` / ``wri.networkx_objective`` for the optimal outcomes."""

from __future__ import annotations

import numpy as np

import wide_range_instances as wri
from network_flow_solver_amd.generators import ArcSoA

MCF_INF = wri.MCF_INF
INT64_MAX = (1 << 63) - 1
FAR = (-1, 1 << 60, 1 << 62, INT64_MAX)        # the encodings of "uncapacitated" (include/mcf.h: cap < 0 or cap >= 2^60)
EDGE_CAP = (1 << 60) - 1                        # the largest capacity that is a bound
EDGE_MIN_COST = 20000                           # only arcs at least this dear get EDGE_CAP (see the module docstring)
LONG_CYCLE = 6000                               # longer than the LDS hit list (4 096) and the LDS path buffers (512) of the
#                                                 cycle scan: the length test_cycle_scan_with_cycles_longer_than_the_lds_buffers uses
PATH_BUFFER_CYCLE = 600                         # longer than the path buffers alone; fits 1 024 nodes
SIZES = {"small": (60, 500), "medium": (1024, 8192), "scale": (40000, 320000)}
INFEASIBLE_VARIANTS = ("starved", "isolated", "cut")


def is_uncapacitated(cap) -> np.ndarray:
    cap = np.asarray(cap, np.int64)
    return (cap < 0) | (cap >= MCF_INF)


def _assert_flow_domain(cap, supply):
    finite = [int(c) for c in np.asarray(cap).tolist() if 0 <= c < (1 << 59)]
    assert sum(finite) + sum(int(s) for s in supply.tolist() if s > 0) < MCF_INF


def uncapacitated(seed: int, n: int = 60, m: int = 500, share: float = 0.4, edge_caps: int = 3, qmax: int = 1 << 40) -> ArcSoA:
    """Feasible and bounded, see the module docstring.  ``edge_caps``: how many arcs get the bound 2^60 - 1."""
    base = wri.make(seed, n, m, qmax)
    rng = np.random.default_rng([20250, seed, n, m])
    cap = base.cap.copy()
    nonneg = np.nonzero(base.cost >= 0)[0]
    pick = rng.choice(nonneg, int(len(nonneg) * share), replace=False)
    cap[pick] = rng.choice(np.array(FAR, np.int64), len(pick))
    dear = np.setdiff1d(np.nonzero(base.cost >= EDGE_MIN_COST)[0], pick)
    assert len(dear) >= edge_caps
    cap[rng.choice(dear, edge_caps, replace=False)] = EDGE_CAP
    assert not is_uncapacitated(cap[base.cost < 0]).any()
    _assert_flow_domain(cap, base.supply)
    return ArcSoA(n, base.tail, base.head, base.cost, cap, base.supply, f"uncap_{n}_{m}_s{seed}")


def unbounded(seed: int, n: int = 60, m: int = 500, cycle_len: int = 5, **kw) -> ArcSoA:
    """``uncapacitated`` plus a planted uncapacitated cycle of cost -1 (its arcs: ``planted(inst, cycle_len)``)."""
    assert 2 <= cycle_len <= n and 3 * cycle_len // 2 + 2 < EDGE_MIN_COST
    base = uncapacitated(seed, n, m, **kw)
    rng = np.random.default_rng([20251, seed, n, m, cycle_len])
    nodes = rng.choice(n, cycle_len, replace=False).astype(np.int32)
    a = rng.integers(1, 4, cycle_len // 2)
    cost = np.zeros(cycle_len, np.int64)
    cost[0:2 * len(a):2], cost[1:2 * len(a):2] = a, -a
    cost[-1] -= 1                                              # (odd length: the last arc costs -1)
    assert int(cost.sum()) == -1 and (cost > 0).any() and (cost < 0).any()
    cap = rng.choice(np.array(FAR, np.int64), cycle_len)
    return ArcSoA(n, np.concatenate((base.tail, nodes)), np.concatenate((base.head, np.roll(nodes, -1))),
                  np.concatenate((base.cost, cost)), np.concatenate((base.cap, cap)), base.supply,
                  f"unbounded_{n}_{m}_c{cycle_len}_s{seed}")


def planted(inst: ArcSoA, cycle_len: int) -> np.ndarray:
    return np.arange(inst.m - cycle_len, inst.m)


def cut_set(inst: ArcSoA) -> np.ndarray:
    """The node set S of the "cut" variant: the longest ring interval of at most n / 4 nodes that holds the largest source
    and has a positive net supply (the first such start; the source alone always qualifies)."""
    n, src = inst.n, int(np.argmax(inst.supply))
    for length in range(max(1, n // 4), 0, -1):
        for back in range(length):
            nodes = (src - back + np.arange(length)) % n
            if int(inst.supply[nodes].sum()) > 0:
                return nodes
    raise AssertionError("unreachable: the source alone has a positive supply")


def infeasible(seed: int, n: int = 60, m: int = 500, variant: str = "starved", **kw) -> ArcSoA:
    """* "starved": the arcs into the largest sink are capped to 0, except (at most) two -- never all -- that together carry
      less than its demand;
    * "isolated": those arcs are removed;
    * "cut": S = ``cut_set``; every arc leaving S is capped to 0 except the ring arc out of its last node, which gets half
      of S's net supply.  That cut is then saturated at every optimum of the big-M problem: while it is not, S holds a node
      whose artificial arc carries excess and the rest a node whose artificial arc carries a deficit (conservation over
      S), the ring -- 8 qmax per arc, more than the whole supply -- leads from the first to the cut arc inside S and from
      its head to the second outside, and that path costs less than n cmax < big-M against the 2 big-M it saves."""
    base = uncapacitated(seed, n, m, **kw)
    tail, head, cost, cap = base.tail, base.head, base.cost, base.cap.copy()
    sink = int(np.argmin(base.supply))
    demand = -int(base.supply[sink])
    into = np.nonzero(head == sink)[0]
    if variant == "starved":
        cap[into] = 0
        cap[into[len(into) - min(2, len(into) - 1):]] = demand // 3      # (the ring arc into the sink is the last of them)
        assert sum(int(c) for c in cap[into].tolist()) < demand and (cap[into] == 0).any()
    elif variant == "isolated":
        keep = head != sink
        tail, head, cost, cap = tail[keep], head[keep], cost[keep], cap[keep]
    elif variant == "cut":
        nodes = cut_set(base)
        inside = np.zeros(n, bool)
        inside[nodes] = True
        leaving = inside[tail] & ~inside[head]
        ring_out = base.m - n + int(nodes[-1])                # wri.make: the ring arc v -> v + 1 is arc m + v
        assert leaving[ring_out] and tail[ring_out] == nodes[-1]
        cap[leaving] = 0
        cap[ring_out] = int(base.supply[nodes].sum()) // 2
        assert sum(int(c) for c in cap[leaving].tolist()) < int(base.supply[nodes].sum())
    else:
        raise ValueError(variant)
    _assert_flow_domain(cap, base.supply)
    return ArcSoA(n, tail, head, cost, cap, base.supply, f"infeasible_{variant}_{n}_{m}_s{seed}")


def cut_of(inst: ArcSoA):
    """(arcs leaving S, the cut's capacity, S's net supply) of an ``infeasible(..., "cut")`` instance."""
    nodes = cut_set(inst)
    inside = np.zeros(inst.n, bool)
    inside[nodes] = True
    leaving = np.nonzero(inside[inst.tail] & ~inside[inst.head])[0]
    assert not is_uncapacitated(inst.cap[leaving]).any()
    return leaving, sum(int(c) for c in inst.cap[leaving].tolist()), int(inst.supply[nodes].sum())


def deep_unbounded(n: int = 48, chain_cost: int = 1000, qmax: int = 1 << 40) -> ArcSoA:
    """In the spirit of ``wri.chain_instance``: an uncapacitated chain 0 -> 1 -> ... -> n-1 of arcs of cost C that carries the
    only supply, and an uncapacitated arc n-1 -> 0 of cost -(n - 1) C - 1.  While a chain arc is missing from the basis
    the return arc prices out (its cycle passes two artificial arcs: -(n - 1) C - 1 + 2 big-M > 0); the chain becomes basic
    from its far end, one arc per pivot, and pivot n closes the cycle of all n arcs, cost -1, no bound: the verdict pivot's
    cycle has n - 1 tree arcs, its end points sit n - 1 levels apart, no depth gate climbs that."""
    C = int(chain_cost)
    assert (n - 1) * C + 1 <= wri.cmax_for(n)
    tail = np.concatenate((np.arange(n - 1), [n - 1])).astype(np.int32)
    head = np.concatenate((np.arange(1, n), [0])).astype(np.int32)
    cost = np.concatenate((np.full(n - 1, C), [-(n - 1) * C - 1])).astype(np.int64)
    cap = np.array([FAR[i % 4] for i in range(n)], np.int64)
    supply = np.zeros(n, np.int64)
    supply[0], supply[n - 1] = qmax - 1, -(qmax - 1)
    return ArcSoA(n, tail, head, cost, cap, supply, f"deep_unbounded_{n}")


def plain_encoding(inst: ArcSoA) -> ArcSoA:
    """The same instance with every uncapacitated arc written as -1 (what the shim's problem classes accept)."""
    return ArcSoA(inst.n, inst.tail, inst.head, inst.cost, np.where(is_uncapacitated(inst.cap), -1, inst.cap), inst.supply, inst.name)


# ------------------------------------------------------------------ exact yardsticks (Python ints only)
def big_m(inst) -> int:
    return wri.big_m_of(inst.n, int(np.abs(inst.cost).max()))


def cycle_of(inst, parent, pred_arc, arc: int):
    """The cycle the non-basic arc `arc`, pushed forward, closes with the tree: [(arc, forward?)] in push order -- `arc`
    itself, from its head up to the join, from the join down to its tail.  parent / pred_arc as mcf_get_tree gives them
    (caller's arc numbers; m + v: the artificial arc of node v)."""
    parent, pred_arc = np.asarray(parent).tolist(), np.asarray(pred_arc).tolist()
    tail, head = inst.tail, inst.head
    u, w = int(head[arc]), int(tail[arc])

    def to_root(v):
        out = [v]
        while parent[v] >= 0:
            v = parent[v]
            out.append(v)
        return out
    pu, pw = to_root(u), to_root(w)
    while len(pu) > 1 and len(pw) > 1 and pu[-2] == pw[-2]:
        pu.pop()
        pw.pop()
    assert pu[-1] == pw[-1]                                    # the join
    cycle = [(int(arc), True)]
    for v in pu[:-1]:                                          # up: v -> parent
        a = pred_arc[v]
        cycle.append((a, a < inst.m and int(tail[a]) == v and int(head[a]) == parent[v]))
    for v in reversed(pw[:-1]):                                # down: parent -> v
        a = pred_arc[v]
        cycle.append((a, a < inst.m and int(tail[a]) == parent[v] and int(head[a]) == v))
    return cycle


def unbounded_certificate(inst, tree, arc: int, rc: int) -> int:
    """The verdict proves itself: the reported arc closes, with the tree, a cycle every arc of which is a real arc
    traversed forward and uncapacitated, of total cost `rc` < 0.  Returns the cycle's length."""
    assert 0 <= arc < inst.m
    cycle = cycle_of(inst, tree["parent"], tree["pred_arc"], arc)
    assert len({a for a, _ in cycle}) == len(cycle) >= 2
    for a, forward in cycle:
        assert a < inst.m, f"artificial arc {a} on the cycle"
        assert forward, f"arc {a} is traversed against its direction: bounded by its flow"
        assert is_uncapacitated(inst.cap[a]), f"arc {a} has the capacity {inst.cap[a]}"
    assert sum(int(inst.cost[a]) for a, _ in cycle) == int(rc) < 0
    return len(cycle)


def _graph(inst, extended: bool):
    import networkx as nx

    g = nx.MultiDiGraph()
    for v, s in enumerate(inst.supply.tolist()):
        g.add_node(v, demand=-int(s))
    for t, h, c, cp in zip(inst.tail.tolist(), inst.head.tolist(), inst.cost.tolist(), inst.cap.tolist()):
        if 0 <= cp < MCF_INF:
            g.add_edge(t, h, weight=int(c), capacity=int(cp))
        else:
            g.add_edge(t, h, weight=int(c))
    if extended:
        g.add_node("root", demand=0)
        for v in range(inst.n):
            g.add_edge(v, "root", weight=big_m(inst))
            g.add_edge("root", v, weight=big_m(inst))
    return g


def networkx_verdict(inst) -> str:
    """An independent verdict from networkx on Python ints: "unbounded" when the uncapacitated arcs alone hold a cycle of
    negative cost (Bellman-Ford, networkx.negative_edge_cycle; every instance here that has one is feasible by
    construction: it is a feasible instance plus arcs), else network_simplex: "infeasible" (NetworkXUnfeasible) or
    "optimal".  network_simplex itself is not asked about the unbounded instances: it raises NetworkXUnbounded on most of
    them but does not come back at all on others (``unbounded(2, 60, 500, 5)`` is one)."""
    import networkx as nx

    free = nx.DiGraph()
    free.add_nodes_from(range(inst.n))
    for t, h, c, cp in zip(inst.tail.tolist(), inst.head.tolist(), inst.cost.tolist(), inst.cap.tolist()):
        if not 0 <= cp < MCF_INF and (not free.has_edge(t, h) or free[t][h]["weight"] > c):
            free.add_edge(t, h, weight=int(c))
    if nx.negative_edge_cycle(free, weight="weight"):
        return "unbounded"
    try:
        nx.network_simplex(_graph(inst, False))
    except nx.NetworkXUnfeasible:
        return "infeasible"
    return "optimal"


def infeasibility_truth(inst, kept=None):
    """networkx.network_simplex on the instance extended by a root node and artificial arcs of cost big-M: (optimum,
    flow on the artificial arcs at that optimum).  ``kept=None``: arcs v -> root and root -> v at every node.  ``kept`` = a
    set of nodes: only the engine's own artificial arc of those nodes (include/mcf.h, mcf_create: ONE per node, v -> root
    for a supply >= 0, root -> v for a demand)."""
    import networkx as nx

    g, M = _graph(inst, False), big_m(inst)
    g.add_node("root", demand=0)
    for v in range(inst.n):
        if kept is None or (v in kept and inst.supply[v] >= 0):
            g.add_edge(v, "root", weight=M)
        if kept is None or (v in kept and inst.supply[v] < 0):
            g.add_edge("root", v, weight=M)
    value, flows = nx.network_simplex(g)
    assert isinstance(value, int)
    art = sum(sum(f.values()) for f in flows["root"].values()) + sum(sum(flows[v]["root"].values()) for v in range(inst.n) if "root" in flows[v])
    return value, art


def check_infeasible(inst, objective: int, artificial_flow: int, tree) -> int:
    """An "infeasible" verdict against networkx, exactly.  The engine, like the reference, never prices an artificial arc
    again once it has left the basis, so where it stops depends on WHICH artificial arcs are left -- rule by rule -- and
    objective + big-M * artificial_flow is not one number per instance.  What holds exactly, and is asserted:
    * the flow left on artificial arcs is the smallest possible: that of the optimum with both artificial arcs at every node;
    * objective + big-M * artificial_flow is no less than that optimum, and EQUALS the optimum of the instance extended by
      just the artificial arcs that are still basic -- the final state is optimal for the problem the engine still holds."""
    assert artificial_flow > 0
    full, least = infeasibility_truth(inst)
    assert artificial_flow == least
    total = objective + big_m(inst) * artificial_flow
    assert total >= full
    basic = {v for v in range(inst.n) if tree["pred_arc"][v] >= inst.m}
    held, art = infeasibility_truth(inst, basic)
    assert total == held and art == artificial_flow
    return total - full


# ------------------------------------------------------------------ the instances the GPU file runs (and the CPU file vets)
def gpu_instances(size: str) -> dict:
    """name -> (instance, expected verdict, planted cycle length or 0)."""
    n, m = SIZES[size]
    if size == "small":
        return {"uncap_0": (uncapacitated(0, n, m), "optimal", 0), "uncap_1": (uncapacitated(1, n, m), "optimal", 0),
                "unbounded_2": (unbounded(0, n, m, 2), "unbounded", 2), "unbounded_5": (unbounded(1, n, m, 5), "unbounded", 5),
                "unbounded_5b": (unbounded(2, n, m, 5), "unbounded", 5), "deep_unbounded": (deep_unbounded(), "unbounded", 0),
                "starved": (infeasible(0, n, m, "starved"), "infeasible", 0), "isolated": (infeasible(1, n, m, "isolated"), "infeasible", 0),
                "cut": (infeasible(2, n, m, "cut"), "infeasible", 0)}
    assert size == "medium"
    return {"uncap_0": (uncapacitated(0, n, m), "optimal", 0), "unbounded_5": (unbounded(0, n, m, 5), "unbounded", 5),
            "unbounded_600": (unbounded(1, n, m, PATH_BUFFER_CYCLE), "unbounded", PATH_BUFFER_CYCLE),
            "cut": (infeasible(0, n, m, "cut"), "infeasible", 0), "starved": (infeasible(1, n, m, "starved"), "infeasible", 0)}
