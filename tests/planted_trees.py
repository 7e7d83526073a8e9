"""Planted spanning forests for the post-solve device passes (``mcf_update_costs``, ``mcf_update_rhs``, ``mcf_certify``,
``mcf_bottlenecks``, ``mcf_certify_ray``, ``mcf_certify_cut``), with every answer known from the construction.  A plain helper
like ``verdict_instances.py``: seeded, numpy plus Python ints, no fixtures.

``mcf_set_basis`` installs any spanning forest the caller names without a pivot, so shape, size and depth of the tree are
chosen here instead of being whatever a solve leaves:

* shapes (``SHAPES``): ``path`` (depth n), ``star`` (depth 1 below its centre), ``caterpillar`` (a spine of n / 2 nodes, a leg
  on each), ``binary`` (balanced), ``random`` (random recursive tree), ``forest`` (k random recursive trees over contiguous node
  ranges).  ``parent[v] < v`` throughout, so every component's lowest node is its top -- the node ``mcf_apply_basis`` hangs a
  component on when no basic arc sits on a bound.  Arc directions are random: tree arcs point towards and away from the root.
* FLOWS ARE PLANTED FIRST, supplies follow from conservation.  Tree flows lie strictly inside (0, cap), or are > 0 on an
  uncapacitated arc (encodings -1, 2^60, 2^62, INT64_MAX), so no basic arc is degenerate and the basis is kept whole; non-tree
  arcs sit at zero or -- ``at_upper`` -- at their capacity; the artificial arc of a component's top carries a planted amount
  (the amounts sum to zero; a single component carries none).
* magnitudes: ``small`` (every value below 2^20) and ``wide`` (``forest`` only): pairs of chords ``at_upper`` of about 2^58 run
  from the LAST node of each component of the upper half to the last node of a component of the lower half, and the tree
  arcs between that node and its component's top are uncapacitated, point the way the chords' flow has to go and carry it.
  Every component of the lower half then has a surplus of about 2^59, all of one sign: the running sum of the node balances
  over the preorder passes 2^64 (asserted) while every arc flow stays below 2^60 and the supplies stay small (asserted: the
  positive ones sum below 2^60, for every variant).
* a second planted flow vector on the same basis (``flow2``, ``art2``, ``supply2``) for ``mcf_update_rhs``, and the same with
  defects (``flow3``, ``supply3``): ``p`` tree arcs pushed out of their bounds and ``q`` basic arcs put on a bound.

Expected answers are exact: numpy int64 where the values fit, limb-split sums and Python ints beyond."""

from __future__ import annotations

import dataclasses

import numpy as np

import verdict_instances as vi
from network_flow_solver_amd.generators import ArcSoA

MCF_INF = 1 << 60
INT64_MAX = (1 << 63) - 1
SHAPES = ("path", "star", "caterpillar", "binary", "random", "forest")
SMALL = 1 << 19                 # small magnitudes: flows, capacities below 2^19, so any node's supply stays below 2^20 per arc
WIDE = 1 << 58
RAY_FIELDS = ("arc", "entering_backward", "length", "join", "backward_count", "capped_count", "artificial_count", "cost",
              "reduced_cost", "theta", "theta_arc", "proven")
CUT_FIELDS = ("seeds", "nodes_in_S", "rounds", "deficit_in_S", "leaving_arcs", "leaving_uncapacitated", "leaving_unsaturated",
              "entering_with_flow", "capacity", "supply", "excess", "artificial_out", "proven")


# ------------------------------------------------------------------ exact sums on numpy arrays
def exact_sum(x) -> int:
    """Sum of an int64 array as a Python int (two 32-bit limbs: no partial sum can wrap below 2^31 entries)."""
    x = np.asarray(x, np.int64)
    return (int((x >> 32).sum()) << 32) + int((x & 0xffffffff).sum())


def exact_dot(x, y) -> int:
    """Sum of x * y as a Python int, |x| and |y| below 2^63 (16-bit limbs: every partial sum stays below 2^63 up to 2^30 entries)."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    total = 0
    for i in range(4):
        xi = (x >> (16 * i)) & 0xffff if i < 3 else x >> 48
        for j in range(4):
            yj = (y >> (16 * j)) & 0xffff if j < 3 else y >> 48
            total += int((xi * yj).sum()) << (16 * (i + j))
    return total


def exact_balances(n: int, tail, head, flow, start) -> list:
    """start[v] - outflow + inflow per node as Python ints (flows of up to 63 bits on any number of arcs)."""
    flow = np.asarray(flow, np.int64)
    hi, lo = np.zeros(n, np.int64), np.zeros(n, np.int64)
    fh, fl = flow >> 30, flow & ((1 << 30) - 1)
    np.subtract.at(hi, tail, fh)
    np.add.at(hi, head, fh)
    np.subtract.at(lo, tail, fl)
    np.add.at(lo, head, fl)
    if np.abs(hi).max(initial=0) < (1 << 31):
        return (np.asarray(start, np.int64) + (hi << 30) + lo).tolist()
    return [int(s) + (int(h) << 30) + int(l) for s, h, l in zip(np.asarray(start).tolist(), hi.tolist(), lo.tolist())]


def first_worst(mask, mag):
    """(count, worst magnitude, lowest index attaining it) of the entries of `mag` selected by `mask`."""
    if not mask.any():
        return 0, 0, -1
    w = int(mag[mask].max())
    return int(mask.sum()), w, int(np.flatnonzero(mask & (mag == w))[0])


def np_cert(inst, cost, flow, pi):
    """The primal / dual groups and the objectives of mcf_certify for caller's arrays (no artificial arcs)."""
    flow = np.asarray(flow, np.int64)
    pi = np.asarray(pi, np.int64)
    cost = np.asarray(cost, np.int64)
    capped = (inst.cap >= 0) & (inst.cap < MCF_INF)
    neg = flow < 0
    over = capped & (flow > inst.cap) & ~neg
    _, bw, bi = first_worst(neg | over, np.where(neg, -flow, flow - np.where(capped, inst.cap, 0)))
    bal = exact_balances(inst.n, inst.tail, inst.head, flow, inst.supply)
    absbal = [abs(b) for b in bal]
    iw = max(absbal) if absbal else 0
    rc = cost + pi[inst.tail] - pi[inst.head]
    lo = (rc < 0) & (~capped | (flow < inst.cap))
    up = (rc > 0) & (flow > 0)
    ln, lw, li = first_worst(lo, -rc)
    un, uw, ui = first_worst(up, rc)
    primal = exact_dot(flow, cost)
    k = capped & (rc < 0)
    dual = -exact_dot(pi[: inst.n], inst.supply) + exact_dot(rc[k], inst.cap[k])
    return {"negative_flow_count": int(neg.sum()), "over_capacity_count": int(over.sum()), "bounds_worst": bw, "bounds_worst_arc": bi,
            "imbalance_count": sum(1 for b in bal if b), "imbalance_worst": min(iw, (1 << 63) - 1),
            "imbalance_worst_node": absbal.index(iw) if iw else -1,
            "dual_lower_count": ln, "dual_lower_worst": lw, "dual_lower_arc": li,
            "dual_upper_count": un, "dual_upper_worst": uw, "dual_upper_arc": ui,
            "primal": primal, "dual": dual, "gap": primal - dual,
            "saturated_arcs": int((capped & (flow == inst.cap) & (flow > 0)).sum())}


# ------------------------------------------------------------------ the planted instance
@dataclasses.dataclass
class Planted:
    inst: ArcSoA
    in_tree: np.ndarray      # bool[m]
    at_upper: np.ndarray     # bool[m]
    flow: np.ndarray         # int64[m]  planted flows: the flows mcf_set_basis has to arrive at
    art: np.ndarray          # int64[n]  planted flow of every node's artificial arc, > 0 node -> root (0 off the components' tops)
    parent: np.ndarray       # int32[n]  planted parent, n (the root) for the top of a component
    tree_arc: np.ndarray     # int64[n]  the node's tree arc (caller's index), m + v for the top of a component
    wide_path: np.ndarray    # bool[m]   tree arcs that carry a wide amount
    supply2: np.ndarray = None
    flow2: np.ndarray = None     # the second vector
    art2: np.ndarray = None
    supply3: np.ndarray = None   # the second vector with defects: flow3 is what conservation gives, out of bounds where planted
    flow3: np.ndarray = None
    out_of_bounds: np.ndarray = None   # arcs of the p defects
    on_bound: np.ndarray = None        # arcs of the q defects
    args: dict = None                  # what plant() was called with

    @property
    def n(self):
        return self.inst.n

    @property
    def m(self):
        return self.inst.m

    @property
    def state(self) -> np.ndarray:
        """What mcf_get_tree reports: 0 basic, -1 non-basic at capacity, 1 non-basic at zero."""
        return np.where(self.in_tree, 0, np.where(self.at_upper, -1, 1)).astype(np.int8)

    @property
    def capped(self) -> np.ndarray:
        return (self.inst.cap >= 0) & (self.inst.cap < MCF_INF)


def shape_parents(shape: str, n: int, rng, k: int = 3) -> np.ndarray:
    """parent[v] < v for every node but the tops of the components, which get -1."""
    v = np.arange(n, dtype=np.int64)
    if shape == "path":
        parent = v - 1
    elif shape == "star":
        parent = np.where(v > 0, 0, -1)
    elif shape == "caterpillar":
        spine = (n + 1) // 2
        parent = np.where(v < spine, v - 1, v - spine)
    elif shape == "binary":
        parent = (v - 1) // 2
    elif shape in ("random", "forest"):
        k = 1 if shape == "random" else max(1, min(k, n))
        start = (np.arange(k + 1, dtype=np.int64) * n) // k          # component c: nodes start[c] .. start[c + 1] - 1
        lo = start[np.searchsorted(start, v, side="right") - 1]
        parent = lo + (rng.random(n) * (v - lo)).astype(np.int64)     # uniform over lo .. v - 1
        parent[v == lo] = -1
    else:
        raise ValueError(shape)
    parent = np.asarray(parent, np.int64)
    assert (parent < v).all() and (parent >= -1).all()
    return parent


def _far(rng, count):
    return rng.choice(np.array(vi.FAR, np.int64), count)


def plant(shape: str, n: int, m: int | None = None, seed: int = 0, magnitude: str = "small", k: int = 3, upper_share: float = 0.4,
          parent=None, art=None, art2=None, chords=None, p: int = 0, q: int = 0) -> Planted:
    """One planted instance, see the module docstring.  ``m``: arcs in all (at least the tree's; default: twice the nodes).
    ``parent`` / ``art`` / ``art2``: a forest and artificial flows of the caller's own.  ``chords``: (tail, head) pairs that
    become the FIRST non-tree arcs.  ``p`` / ``q``: defects of the second vector."""
    args = dict(shape=shape, n=n, m=m, seed=seed, magnitude=magnitude, k=k, upper_share=upper_share, parent=parent, art=art, art2=art2, chords=chords)
    rng = np.random.default_rng([20260, SHAPES.index(shape) if shape in SHAPES else 9, n, seed, 0 if magnitude == "small" else 1])
    wide = magnitude == "wide"
    assert magnitude in ("small", "wide") and (not wide or shape == "forest")
    parent = shape_parents(shape, n, rng, k) if parent is None else np.asarray(parent, np.int64)
    tops = np.flatnonzero(parent < 0)
    child = np.flatnonzero(parent >= 0)
    ntree = len(child)
    extra_fixed = 0 if chords is None else len(chords)
    if m is None:
        m = max(2 * n, ntree + extra_fixed) if n > 1 else 0
    extra = m - ntree
    assert extra >= extra_fixed and (n > 1 or m == 0)
    # ---- arcs: the tree's, then the others; a random order in the end
    up = rng.random(ntree) < 0.5                                     # tail = child
    t_tree, h_tree = np.where(up, child, parent[child]), np.where(up, parent[child], child)
    t_x = rng.integers(0, n, extra)
    h_x = (t_x + 1 + rng.integers(0, max(n - 1, 1), extra)) % n if n > 1 else t_x
    if extra_fixed:
        t_x[:extra_fixed], h_x[:extra_fixed] = np.asarray(chords, np.int64).T
    cap = np.empty(m, np.int64)
    flow = np.zeros(m, np.int64)
    uncapped = rng.random(ntree) < 0.5
    cap[:ntree] = np.where(uncapped, _far(rng, ntree), rng.integers(2, SMALL, ntree))
    tree_hi = np.where(uncapped, SMALL, cap[:ntree])                 # flows in [1, hi - 1]

    def tree_flows():
        return 1 + (rng.random(ntree) * (tree_hi - 1)).astype(np.int64)
    flow[:ntree] = tree_flows()
    x_upper = rng.random(extra) < upper_share
    if extra_fixed:
        x_upper[0] = True                                            # (the first chord sits at its capacity: a ray entered backward)
        x_upper[1:extra_fixed] = False
    cap[ntree:] = np.where(x_upper | (rng.random(extra) < 0.5), rng.integers(1, SMALL, extra), _far(rng, extra))
    flow[ntree:] = np.where(x_upper, cap[ntree:], 0)
    cost = rng.integers(-1000, 1001, m)
    tail, head = np.concatenate((t_tree, t_x)), np.concatenate((h_tree, h_x))
    in_tree = np.arange(m) < ntree
    at_upper = np.concatenate((np.zeros(ntree, bool), x_upper))
    tree_arc = np.full(n, -1, np.int64)
    tree_arc[child] = np.arange(ntree)
    wide_part = np.zeros(m, np.int64)
    wide_art = np.zeros(n, np.int64)
    if wide:
        # chords: components of the upper half send, those of the lower half receive, two chords each, last node to last node
        ncomp = len(tops)
        half = ncomp // 2
        assert half >= 40 and extra >= 2 * half
        last = np.append(tops[1:], n) - 1
        slot = ntree
        for c in range(half):
            snd, rcv = int(last[half + c]), int(last[c])
            for j in range(2):
                w = WIDE - int(rng.integers(0, SMALL))
                tail[slot], head[slot], cap[slot], flow[slot], at_upper[slot] = snd, rcv, w, w, True
                slot += 1
                for end, towards_top in ((rcv, True), (snd, False)):   # the receiver passes it up to its top, the sender draws it down
                    u = end
                    while parent[u] >= 0:
                        a = tree_arc[u]
                        tail[a], head[a] = (u, parent[u]) if towards_top else (parent[u], u)
                        if not uncapped[a]:
                            cap[a], uncapped[a] = -1, True
                            tree_hi[a] = SMALL
                            flow[a] = 1 + flow[a] % (SMALL - 1)
                        wide_part[a] += w
                        u = int(parent[u])
                    wide_art[u] += w if towards_top else -w
        flow += wide_part
    # ---- artificial flows of the tops: planted, summing to zero
    def art_flows(given):
        a = np.zeros(n, np.int64)
        if given is not None:
            a[:] = given
        elif len(tops) > 1:
            a[tops[:-1]] = rng.integers(1, SMALL, len(tops) - 1) * rng.choice(np.array([-1, 1]), len(tops) - 1)
            a[tops[-1]] = -a.sum()
        assert a.sum() == 0 and not a[child].any()
        return a + wide_art
    art_v = art_flows(art)
    perm = rng.permutation(m)
    inv = np.empty(m, np.int64)
    inv[perm] = np.arange(m)
    tail, head, cost, cap, flow, in_tree, at_upper, wide_part = (a[perm] for a in (tail, head, cost, cap, flow, in_tree, at_upper, wide_part))
    tree_arc = np.where(tree_arc >= 0, np.append(inv, 0)[np.maximum(tree_arc, 0)], m + np.arange(n))

    def supplies(f, a):
        s = a.copy()
        np.add.at(s, tail, f)
        np.subtract.at(s, head, f)
        return s
    supply = supplies(flow, art_v)
    inst = ArcSoA(n, tail.astype(np.int32), head.astype(np.int32), cost, cap, supply, f"planted_{shape}_{n}_{m}_{magnitude}_s{seed}")
    pl = Planted(inst, in_tree, at_upper, flow, art_v, np.where(parent < 0, n, parent).astype(np.int32), tree_arc, wide_part != 0)
    # ---- the second vector on the same basis
    flow2 = flow.copy()
    tree_ids = inv[:ntree]                                           # (caller's index of tree arc i of the construction)
    flow2[tree_ids] = tree_flows() + wide_part[tree_ids]
    pl.flow2, pl.art2 = flow2, art_flows(art2)
    pl.supply2 = supplies(flow2, pl.art2)
    # ---- ... and the second vector with defects (drawn last: instance and both clean vectors do not depend on p and q)
    free = tree_ids[~pl.wide_path[tree_ids]]
    assert p + q <= len(free)
    pick = rng.choice(free, p + q, replace=False) if p + q else np.zeros(0, np.int64)
    pl.out_of_bounds, pl.on_bound = pick[:p], pick[p:]
    flow3 = flow2.copy()
    for i, a in enumerate(pl.out_of_bounds):                         # above the capacity where there is one, else negative
        flow3[a] = cap[a] + 1 + i if (pl.capped[a] and i % 2 == 0) else -1 - i
    for i, a in enumerate(pl.on_bound):
        flow3[a] = cap[a] if (pl.capped[a] and i % 2 == 0) else 0
    pl.flow3, pl.supply3 = flow3, supplies(flow3, pl.art2)
    pl.args = args
    check_planted(pl, wide)
    return pl


def plant_defects(pl: Planted, p: int, q: int) -> Planted:
    """The same instance, basis and clean vectors, with other defects in the third vector."""
    return plant(**pl.args, p=p, q=q)


def check_planted(pl: Planted, wide: bool = False) -> None:
    """The construction's own promises: conservation, bounds, no degenerate basic arc, the numeric domain."""
    inst, f = pl.inst, pl.flow
    for supply, flow, art, defects in ((inst.supply, pl.flow, pl.art, False), (pl.supply2, pl.flow2, pl.art2, False), (pl.supply3, pl.flow3, pl.art2, True)):
        bal = exact_balances(inst.n, inst.tail, inst.head, flow, supply)
        assert bal == pl_list(art), "conservation"
        assert exact_sum(supply) == 0 and exact_sum(supply[supply > 0]) < MCF_INF
        assert (np.abs(art) < MCF_INF).all()
        ok = np.ones(inst.m, bool)
        if defects:
            ok[pl.out_of_bounds] = False
            ok[pl.on_bound] = False
        t = pl.in_tree & ok
        assert (flow[t] > 0).all() and (flow[t] < np.where(pl.capped, inst.cap, MCF_INF)[t]).all(), "a basic arc on a bound"
        assert (flow[~pl.in_tree] == np.where(pl.at_upper, inst.cap, 0)[~pl.in_tree]).all()
    assert int(pl.in_tree.sum()) == int((pl.parent < inst.n).sum()) and not (pl.in_tree & pl.at_upper).any()
    assert pl.capped[pl.at_upper].all() and (inst.cap[pl.at_upper] > 0).all()
    if wide:
        assert max_prefix(pl, pl.art) > 1 << 64 and max_prefix(pl, pl.art2) > 1 << 64 and (f < MCF_INF).all()
    else:
        assert (np.abs(f) < 2 * SMALL).all() and (np.abs(inst.cost) < 2 * SMALL).all()


def pl_list(a) -> list:
    return [int(x) for x in np.asarray(a).tolist()]


def max_prefix(pl: Planted, art) -> int:
    """Greatest |running sum| of the node balances at the ends of the components, in the order of the preorder (components in
    node order, each one whole): a component's balances add up to what its artificial arc carries."""
    run, worst = 0, 0
    for a in pl_list(art[pl.parent == pl.n]):
        run += a
        worst = max(worst, abs(run))
    return worst


# ------------------------------------------------------------------ expected answers
def check_tree_arrays(n: int, parent, size, pos, order, depth, psize=None) -> None:
    """conftest.check_tree_invariants on whole arrays (the same statements; for trees of millions of nodes)."""
    N = n + 1
    parent, size, pos, order, depth = (np.asarray(a, np.int64) for a in (parent, size, pos, order, depth))
    assert np.array_equal(np.sort(order), np.arange(N)) and np.array_equal(order[pos], np.arange(N))
    assert parent[n] == -1 and pos[n] == 0 and size[n] == N and depth[n] == 0
    v = np.arange(n)
    pv = parent[v]
    assert ((pv >= 0) & (pv < N)).all()
    assert (pos[pv] < pos[v]).all() and (pos[v] + size[v] <= pos[pv] + size[pv]).all()
    assert np.array_equal(np.bincount(pv, weights=size[v], minlength=N).astype(np.int64) + 1, size)
    assert (depth[v] == depth[pv] + 1).all()
    if psize is not None and not (np.asarray(psize) == -1).all():
        assert np.array_equal(np.asarray(psize, np.int64)[pos], size)


def big_m(pl_or_inst, cost=None) -> int:
    inst = getattr(pl_or_inst, "inst", pl_or_inst)
    c = inst.cost if cost is None else np.asarray(cost)
    return (int(np.abs(c).max(initial=0)) + 1) * (inst.n + 2)


def potentials(pl: Planted, tree: dict, cost, bigm: int, art=None) -> np.ndarray:
    """pi[n + 1] from the orientation the engine reports: root 0, pi[child] = pi[parent] - cost when the child is the tail of its
    tree arc, + cost when it is the head; an artificial arc costs big-M and points node -> root unless it carries flow from the
    root.  A node's term reaches the positions of its subtree: one difference array over the preorder."""
    n, m = pl.n, pl.m
    art = pl.art if art is None else art
    pred = np.asarray(tree["pred_arc"], np.int64)[:n]
    pos, size = np.asarray(tree["pos"], np.int64), np.asarray(tree["size"], np.int64)
    v = np.arange(n)
    real = pred < m
    a = np.where(real, pred, 0)
    tail, head, cost = (np.append(np.asarray(x, np.int64), 0) for x in (pl.inst.tail, pl.inst.head, cost))   # (m = 0: `a` still has to index something)
    is_tail = tail[a] == v
    assert (np.where(is_tail, head[a], tail[a])[real] == np.asarray(tree["parent"])[:n][real]).all()
    term = np.where(real, np.where(is_tail, -cost[a], cost[a]), np.where(art >= 0, -bigm, bigm))
    diff = np.zeros(n + 2, np.int64)
    np.add.at(diff, pos[v], term)
    np.subtract.at(diff, pos[v] + size[v], term)
    at_pos = np.cumsum(diff)[: n + 1]
    return at_pos[pos]


def wrong_way(pl: Planted, tree: dict, arcs, flow) -> int:
    """How many of the basic arcs `arcs` sit on a bound pointing the wrong way: full towards the root, empty away from it."""
    count = 0
    parent = np.asarray(tree["parent"])
    for a in pl_list(arcs):
        t, h = int(pl.inst.tail[a]), int(pl.inst.head[a])
        up = parent[t] == h and int(np.asarray(tree["pred_arc"])[t]) == a
        assert up or (parent[h] == t and int(np.asarray(tree["pred_arc"])[h]) == a)
        f = int(flow[a])
        count += (up and bool(pl.capped[a]) and f == int(pl.inst.cap[a])) or (not up and f == 0)
    return count


def certificate(pl: Planted, cost, flow, pi, art, bigm: int, supply=None) -> dict:
    """Every field of mcf_certify for the RESIDENT state (flows, potentials with the root last, artificial flows) that does not
    depend on the handle's pricing path.  ``artificial_flow`` is the low 64 bits of the sum, as the struct's field is."""
    inst = pl.inst if supply is None else dataclasses.replace(pl.inst, supply=np.asarray(supply, np.int64))
    pi = np.asarray(pi, np.int64)
    d = np_cert(inst, cost, flow, pi[: pl.n] - pi[pl.n])
    bal = exact_balances(inst.n, inst.tail, inst.head, flow, inst.supply)
    bal = [b - a for b, a in zip(bal, pl_list(art))]                 # the artificial arc takes art[v] out of node v
    absbal = [abs(b) for b in bal]
    iw = max(absbal) if absbal else 0
    total = exact_sum(np.abs(art))
    low = ((total + (1 << 63)) % (1 << 64)) - (1 << 63)
    d.update(imbalance_count=sum(1 for b in bal if b), imbalance_worst=min(iw, INT64_MAX), imbalance_worst_node=absbal.index(iw) if iw else -1,
             artificial_flow=low, big_m=bigm, bigm_term=bigm * low)
    d["gap"] = d["primal"] + d["bigm_term"] - d["dual"]
    clean = not any(d[k] for k in ("negative_flow_count", "over_capacity_count", "imbalance_count", "dual_lower_count", "dual_upper_count"))
    d["verdict"] = ("infeasible" if low > 0 else "optimal") if clean and d["gap"] == 0 else "not_proven"
    d.update(checks=63, basic_arcs=pl.n, basic_count_mismatch=0, tree_rc_count=0, state_flow_count=0, tree_shape_count=0, strong_count=0,
             rc_mismatch_count=0, key_mismatch_count=0)
    return d


def bottleneck_list(pl: Planted, flow, num: int, den: int) -> np.ndarray:
    """Ascending indices of the capped arcs carrying flow with flow * den >= cap * num (products in Python ints where they need it)."""
    flow = np.asarray(flow, np.int64)
    cand = pl.capped & (flow > 0)
    big = cand & ((flow >= (1 << 56)) | (pl.inst.cap >= (1 << 56)))
    small = cand & ~big
    hit = np.zeros(pl.m, bool)
    hit[small] = flow[small] * den >= pl.inst.cap[small] * num
    for a in np.flatnonzero(big).tolist():
        hit[a] = int(flow[a]) * den >= int(pl.inst.cap[a]) * num
    return np.flatnonzero(hit)


class RayWalker:
    """mcf_certify_ray by walking parent pointers (the lists are taken once per state)."""

    def __init__(self, pl: Planted, tree: dict, cost, flow, pi, art, bigm: int):
        self.n, self.m, self.bigm = pl.n, pl.m, bigm
        self.parent, self.pred = np.asarray(tree["parent"]).tolist(), np.asarray(tree["pred_arc"]).tolist()
        self.T, self.H, self.U = pl.inst.tail.tolist(), pl.inst.head.tolist(), pl.inst.cap.tolist()
        self.C, self.F, self.pi, self.art = pl_list(cost), pl_list(flow), pl_list(pi), pl_list(art)

    def _item(self, v, climbing):
        a = self.pred[v]
        if a < self.m:
            up = self.T[a] == v and self.H[a] == self.parent[v]
            assert up or (self.H[a] == v and self.T[a] == self.parent[v])
            return a, up == climbing, self.C[a], (self.U[a] if 0 <= self.U[a] < MCF_INF else None), self.F[a], False
        assert a == self.m + v and self.parent[v] == self.n
        return a, (self.art[v] >= 0) == climbing, self.bigm, None, abs(self.art[v]), True

    def ray(self, arc: int, backward: bool) -> dict:
        T, H, C, U = self.T, self.H, self.C, self.U
        first, second = (T[arc], H[arc]) if backward else (H[arc], T[arc])

        def to_root(v):
            out = [v]
            while self.parent[v] >= 0:
                v = self.parent[v]
                out.append(v)
            return out
        pu, pw = to_root(first), to_root(second)
        while len(pu) > 1 and len(pw) > 1 and pu[-2] == pw[-2]:
            pu.pop()
            pw.pop()
        assert pu[-1] == pw[-1]
        items = [(arc, not backward, C[arc], (U[arc] if 0 <= U[arc] < MCF_INF else None), self.F[arc], False)]
        items += [self._item(v, True) for v in pu[:-1]] + [self._item(v, False) for v in reversed(pw[:-1])]
        theta, theta_arc = MCF_INF, -1
        for a, fwd, _, cap, f, _ in items:
            residual = (MCF_INF if cap is None else cap - f) if fwd else f
            if residual < MCF_INF and (residual < theta or (residual == theta and a < theta_arc)):
                theta, theta_arc = residual, a
        rc = C[arc] + self.pi[T[arc]] - self.pi[H[arc]]
        d = {"arc": arc, "entering_backward": bool(backward), "length": len(items), "join": pu[-1],
             "backward_count": sum(1 for it in items[1:] if not it[1]), "capped_count": sum(1 for it in items if it[3] is not None),
             "artificial_count": sum(1 for it in items if it[5]), "cost": sum(it[2] if it[1] else -it[2] for it in items),
             "reduced_cost": -rc if backward else rc, "theta": theta, "theta_arc": theta_arc}
        d["proven"] = not backward and d["backward_count"] == d["capped_count"] == d["artificial_count"] == 0 and d["cost"] < 0
        d["arcs"] = [it[0] for it in items]
        return d


def cut_answer(pl: Planted, S, supply=None, flow=None, art=None, rounds: int = 0) -> dict:
    """The fields of mcf_cut for the node set S; flow / art None: the caller's-set mode (the resident fields stay 0)."""
    inst = pl.inst
    S = np.asarray(S, bool)
    supply = inst.supply if supply is None else np.asarray(supply, np.int64)
    tin, hin = S[inst.tail], S[inst.head]
    leave, enter = tin & ~hin, hin & ~tin
    d = dict.fromkeys(CUT_FIELDS, 0)
    d["rounds"] = rounds
    d["leaving_arcs"] = int(leave.sum())
    d["leaving_uncapacitated"] = int((leave & ~pl.capped).sum())
    d["capacity"] = exact_sum(inst.cap[leave & pl.capped])
    if flow is not None:
        flow = np.asarray(flow, np.int64)
        d["leaving_unsaturated"] = int((leave & (~pl.capped | (flow < inst.cap))).sum())
        d["entering_with_flow"] = int((enter & (flow > 0)).sum())
    d["nodes_in_S"] = int(S.sum())
    d["supply"] = exact_sum(supply[S])
    if art is not None:
        art = np.asarray(art, np.int64)
        d["seeds"], d["deficit_in_S"], d["artificial_out"] = int((art[S] > 0).sum()), int((art[S] < 0).sum()), exact_sum(art[S])
    d["excess"] = d["supply"] - d["capacity"]
    d["proven"] = d["leaving_uncapacitated"] == 0 and d["excess"] > 0
    return d


def residual_levels(pl: Planted, flow, art):
    """(S, levels): breadth-first from the nodes with art > 0 over arcs with room (tail -> head) and arcs carrying flow
    (head -> tail), a frontier at a time.  levels = 1 + the greatest distance from a seed, 0 without seeds."""
    inst, n = pl.inst, pl.n
    flow, art = np.asarray(flow, np.int64), np.asarray(art, np.int64)
    room = ~pl.capped | (flow < inst.cap)
    src = np.concatenate((inst.tail[room], inst.head[flow > 0])).astype(np.int64)
    dst = np.concatenate((inst.head[room], inst.tail[flow > 0])).astype(np.int64)
    by = np.argsort(src, kind="stable")
    src, dst = src[by], dst[by]
    off = np.searchsorted(src, np.arange(n + 1))
    dist = np.zeros(n, np.int64)
    front = np.flatnonzero(art > 0)
    dist[front] = 1
    level = 1 if len(front) else 0
    while len(front):
        lo, hi = off[front], off[front + 1]
        cnt = hi - lo
        idx = np.repeat(lo - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(int(cnt.sum()))
        nxt = np.unique(dst[idx])
        nxt = nxt[dist[nxt] == 0]
        if len(nxt):
            level += 1
            dist[nxt] = level
        front = nxt
    return dist > 0, level


def subtree_set(pl: Planted, top: int) -> np.ndarray:
    """The planted subtree below (and with) `top`: parent[v] < v, so one pass in node order."""
    inside = np.zeros(pl.n + 1, bool)
    inside[top] = True
    par = pl.parent.tolist()
    for v in range(top + 1, pl.n):
        inside[v] = inside[par[v]]
    return inside[: pl.n]


# ------------------------------------------------------------------ the 64-bit edge of mcf_apply_basis
def int64_edge(arcs_at_upper: int, shared_return: bool):
    """One node (0) with k = `arcs_at_upper` outgoing non-basic arcs at capacity 2^60 - 1, to the nodes 1 .. k.  Either every one
    returns through its own uncapacitated tree arc i -> 0 (valid: every flow below 2^60), or every node i passes it on to a hub
    k + 1 whose uncapacitated tree arc hub -> 0 has to return all of it: k * (2^60 - 1), outside the domain for any k > 1.
    Node 0's balance leaves int64 from 8 such arcs on; from 16 on a sum of them wraps to a small value.
    Returns (instance, in_tree, at_upper, planted flows or None)."""
    k, big = arcs_at_upper, MCF_INF - 1
    mids = list(range(1, k + 1))
    if shared_return:
        n, hub = k + 2, k + 1
        tail, head = [0] * k + mids + [hub], mids + [hub] * k + [0]
    else:
        n = k + 1
        tail, head = [0] * k + mids, mids + [0] * k
    m = len(tail)
    cap = np.array([big] * k + [-1] * (m - k), np.int64)
    at_upper, in_tree = np.arange(m) < k, np.arange(m) >= k
    supply = np.zeros(n, np.int64)
    supply[0], supply[k] = 5, -5                                      # a little real traffic on top: node k keeps 5 of what it receives
    flow = None
    if not shared_return:
        flow = np.full(m, big, np.int64)
        flow[m - 1] -= 5
    inst = ArcSoA(n, np.array(tail, np.int32), np.array(head, np.int32), np.arange(1, m + 1, dtype=np.int64), cap, supply, f"int64_edge_{k}_{int(shared_return)}")
    return inst, in_tree, at_upper, flow


# ------------------------------------------------------------------ the cases of tests/test_gpu_passes_geometry.py
# (test_planted_trees_cpu.py shows for every one of them that the host code keeps the planted basis whole)
LAYOUTS = (-1, 2, 10)                                   # tree_blocks: dense array, blocks of 4 slots, blocks of 1 024
SWEEP_N = (1, 2, 63, 64, 255, 256, 2047, 2048, 4096)    # n_nodes = n + 1: 2, 3, 64 / 65, 256 / 257 (workgroups), 2 048 / 2 049 (scan chunks), 4 097
SWEEP_SHAPES = ("path", "star", "random", "forest")
DEFECTS = ((1, 0), (1, 2), (3, 0), (3, 2))              # (p, q) of the second vector
DEPTHS = (1, 2, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025)
CUT_CHAINS = (31, 32, 33, 65)
LANE_CAP = 2048 * 256                                   # lanes of a node pass: 2 048 workgroups of 256
LARGE_N = LANE_CAP + 257
SCAN_N = 2048 * 1024 + 2049                             # n_nodes = n + 1 positions: 1 026 scan chunks, the last one holding a single position
NT_ARCS = (1 << 22) + 5


def sweep_cases():
    """(id, n, shape, tree_blocks, m): every size with every shape; layouts and arc counts rotate, so that every size and every
    shape meets every layout and both arc counts."""
    out = []
    for i, n in enumerate(SWEEP_N):
        for j, shape in enumerate(SWEEP_SHAPES):
            tb = LAYOUTS[(i + j) % 3]
            m = 0 if n == 1 else (4096, 4097)[(i + j // 3 + j) % 2]
            out.append((f"n{n}-{shape}-tb{tb}-m{m}", n, shape, tb, m))
    return out


def sweep_plant(n, shape, m, p=0, q=0) -> Planted:
    return plant(shape, n, m, seed=n, k=max(1, min(3, n // 2)), p=p, q=q)


def sweep_defects(pl: Planted):
    """The (p, q) that fit into the tree."""
    return [(p, q) for p, q in DEFECTS if p + q <= int(pl.in_tree.sum())]


def depth_plant(d: int) -> Planted:
    """Greatest depth d (the root at 0): a path of d nodes 0 .. d - 1 below the root, node v at depth v + 1, and two single
    nodes, all three hung on the root.  The first chord joins the deepest node to the node at depth 1 and sits at its capacity,
    the second the same nodes at zero.  Second vector: the path's artificial arc turns round, the other two keep their sign."""
    assert d >= 2
    n = d + 2
    parent = np.arange(n, dtype=np.int64) - 1
    parent[d], parent[d + 1] = -1, -1
    art, art2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    art[[0, d, d + 1]] = 5, -10, 5
    art2[[0, d, d + 1]] = -5, -10, 15
    return plant("path", n, m=(d - 1) + 8, seed=d, parent=parent, art=art, art2=art2, chords=[(d - 1, 0), (d - 1, 0)])


def large_plant(shape: str, p=0, q=0) -> Planted:
    """The shape over all nodes but the last 64, which hang on the root by themselves: artificial arcs that carry flow at nodes
    past the lane cap (a single component's artificial arc carries none)."""
    parent = shape_parents(shape, LARGE_N, np.random.default_rng([7, SHAPES.index(shape)]))
    parent[-64:] = -1
    return plant(shape, LARGE_N, 2 * LARGE_N, seed=7, parent=parent, p=p, q=q)


def scan_plant() -> Planted:
    return plant("forest", SCAN_N, NT_ARCS, seed=11, magnitude="wide", k=96, p=3)


def cold_plant(n: int = 4, m: int = 8) -> Planted:
    """Greatest depth 1: every node hangs on the root and no real arc carries anything -- the cold start of a fresh handle."""
    art = np.zeros(n, np.int64)
    art[:4] = 5, -20, 7, 8
    return plant("forest", n, m, seed=1, k=n, upper_share=0.0, art=art)
