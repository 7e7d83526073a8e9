"""Two independent yardsticks for ``mcf_supply_ranges`` / ``mcf_capacity_ranges`` on numpy arrays / Python ints.  A plain helper
like ``ranges_yardsticks.py``: no fixtures, no device, no code shared with the engine.

The definition (include/mcf.h).  The tree arc of node ``v`` points child -> parent (``up``) or parent -> child and has the
residuals ``with`` = ``cap - flow`` (``INF`` when uncapacitated or artificial) and ``against`` = ``flow``;
``U[v]`` = the residual of a push child -> parent, ``D[v]`` = parent -> child.  ``push(x -> y)`` = min of ``U`` over the tree
arcs from ``x`` up to the join and of ``D`` from the join down to ``y``; ``limit_arc`` = the FIRST arc in push order that
attains it (caller's index, ``m + v`` for an artificial arc, -1 when the limit is ``INF``); ``art_rising`` = artificial arcs
on the path pushed along their direction.

``walk`` / ``walk_one`` climb the parent pointers from both ends by depth; ``by_intervals`` knows no depth: the tree arc of
``u`` is on the path iff exactly one end point lies in ``[pos[u], pos[u] + size[u])``, and nested subtrees order themselves by
size.  They share the residuals (``TreeState``) and nothing else."""

from __future__ import annotations

import dataclasses

import numpy as np

INF = (1 << 63) - 1
MCF_INF = 1 << 60
REPORT = ("basic_real", "basic_artificial", "at_capacity", "max_depth", "levels", "inf_count", "zero_count", "art_rising_count")


@dataclasses.dataclass
class TreeState:
    """A basis with its flows, in the caller's terms.  Node arrays have n + 1 entries (the root is node n)."""
    n: int
    m: int
    tail: np.ndarray
    head: np.ndarray
    cap: np.ndarray          # mcf_create's convention: < 0 or >= 2^60 = uncapacitated
    flow: np.ndarray         # int64[m]
    parent: np.ndarray
    depth: np.ndarray
    pred_arc: np.ndarray     # caller's index of the node's tree arc, m + v for an artificial one, -1 for the root
    art_flow: np.ndarray     # int64[n] magnitude of the flow of node v's artificial arc
    art_up: np.ndarray       # bool[n]  it points v -> root
    pos: np.ndarray = None
    size: np.ndarray = None

    @property
    def capped(self):
        return (self.cap >= 0) & (self.cap < MCF_INF)

    def residuals(self):
        """(U, D, up, artificial) per node 0 .. n - 1."""
        n, m = self.n, self.m
        a = np.asarray(self.pred_arc, np.int64)[:n]
        art = a >= m
        ar = np.where(art, 0, a)
        tail, cap, flow = (np.append(np.asarray(x, np.int64), 0) for x in (self.tail, self.cap, self.flow))   # (m == 0: `ar` still indexes something)
        capped = (cap >= 0) & (cap < MCF_INF)
        up = np.where(art, np.asarray(self.art_up, bool), tail[ar] == np.arange(n))
        with_ = np.where(art | ~capped[ar], INF, cap[ar] - flow[ar])
        against = np.where(art, np.asarray(self.art_flow, np.int64), flow[ar])
        return np.where(up, with_, against), np.where(up, against, with_), up, art


def planted_state(pl, tree) -> TreeState:
    """The planted basis of ``planted_trees`` with its first flow vector; ``tree`` = ``ranges_yardsticks.planted_tree(pl)`` or
    ``mcf_get_tree`` of a handle holding it."""
    inst = pl.inst
    return TreeState(pl.n, pl.m, inst.tail, inst.head, inst.cap, pl.flow, np.asarray(tree["parent"]), np.asarray(tree["depth"]),
                     np.asarray(tree["pred_arc"]), np.abs(pl.art), pl.art >= 0, np.asarray(tree["pos"]), np.asarray(tree["size"]))


def resident_state(inst, tree, flow, supply=None, cap=None) -> TreeState:
    """What a handle holds, from ``mcf_get_tree`` and the flows of ``mcf_get_result``: an artificial arc carries what its
    subtree has left over, and points node -> root exactly when the node's potential lies below the root's."""
    n = inst.n
    supply = inst.supply if supply is None else supply
    cap = inst.cap if cap is None else cap
    flow = np.asarray(flow, np.int64)
    bal = np.asarray(supply, np.int64).copy()
    np.subtract.at(bal, inst.tail, flow)
    np.add.at(bal, inst.head, flow)
    pos, size = np.asarray(tree["pos"], np.int64), np.asarray(tree["size"], np.int64)
    at_pos = np.zeros(n + 2, np.int64)
    at_pos[pos[:n] + 1] = bal
    pre = np.cumsum(at_pos)
    surplus = pre[pos[:n] + size[:n]] - pre[pos[:n]]
    pi = np.asarray(tree["pi"], np.int64)
    return TreeState(n, inst.m, inst.tail, inst.head, np.asarray(cap, np.int64), flow, np.asarray(tree["parent"]), np.asarray(tree["depth"]),
                     np.asarray(tree["pred_arc"]), np.abs(surplus), pi[:n] < pi[n], pos, size)


# ------------------------------------------------------------------ push(x -> y)
def walk_one(st: TreeState, x: int, y: int, res=None) -> tuple:
    """(limit, limit_arc, art_rising) of one pair, the arcs collected in push order."""
    U, D, up, art = st.residuals() if res is None else res
    parent, depth = st.parent, st.depth
    xs, ys = [], []
    a, b = int(x), int(y)
    while depth[a] > depth[b]:
        xs.append(a)
        a = int(parent[a])
    while depth[b] > depth[a]:
        ys.append(b)
        b = int(parent[b])
    while a != b:
        xs.append(a)
        ys.append(b)
        a, b = int(parent[a]), int(parent[b])
    order = [(int(U[v]), v, bool(art[v] and up[v])) for v in xs] + [(int(D[v]), v, bool(art[v] and not up[v])) for v in reversed(ys)]
    limit, arc = INF, -1
    for r, v, _ in order:
        if r < limit:
            limit, arc = r, int(st.pred_arc[v])
    return limit, arc, sum(1 for _, _, rising in order if rising)


def walk(st: TreeState, xs, ys) -> tuple:
    """``walk_one`` for many pairs at once: (limit, limit_arc, art_rising) arrays.  Every round each pair's deeper end (both at
    equal depths) climbs one arc; upwards an earlier arc keeps a tie, downwards a later -- higher -- one takes it."""
    U, D, up, art = (np.append(r, v) for r, v in zip(st.residuals(), (INF, INF, False, False)))
    parent, depth = np.asarray(st.parent, np.int64), np.asarray(st.depth, np.int64)
    a, b = np.asarray(xs, np.int64).copy(), np.asarray(ys, np.int64).copy()
    k = len(a)
    lx, ly = np.full(k, INF, np.int64), np.full(k, INF, np.int64)
    ax, ay = np.full(k, -1, np.int64), np.full(k, -1, np.int64)
    rising = np.zeros(k, np.int32)
    while True:
        live = a != b
        if not live.any():
            break
        go_a, go_b = live & (depth[a] >= depth[b]), live & (depth[b] >= depth[a])
        take = go_a & (U[a] < lx)
        lx, ax = np.where(take, U[a], lx), np.where(take, a, ax)
        take = go_b & (D[b] <= ly)
        ly, ay = np.where(take, D[b], ly), np.where(take, b, ay)
        rising += (go_a & art[a] & up[a]).astype(np.int32) + (go_b & art[b] & ~up[b]).astype(np.int32)
        a, b = np.where(go_a, parent[a], a), np.where(go_b, parent[b], b)
    y_side = ly < lx
    limit, node = np.where(y_side, ly, lx), np.where(y_side, ay, ax)
    arc = np.where(limit == INF, -1, np.append(np.asarray(st.pred_arc, np.int64)[: st.n + 1], -1)[node])
    return limit, arc, rising


def by_intervals(st: TreeState, x: int, y: int, res=None) -> tuple:
    """(limit, limit_arc, art_rising) of one pair without depths: membership by preorder intervals, order by subtree size."""
    U, D, up, art = st.residuals() if res is None else res
    n = st.n
    pos, size = np.asarray(st.pos, np.int64)[:n], np.asarray(st.size, np.int64)[:n]
    has_x = (pos <= st.pos[x]) & (st.pos[x] < pos + size)
    has_y = (pos <= st.pos[y]) & (st.pos[y] < pos + size)
    side_x, side_y = np.flatnonzero(has_x & ~has_y), np.flatnonzero(has_y & ~has_x)
    side_x = side_x[np.argsort(size[side_x])]                 # bottom-up: the subtrees grow
    side_y = side_y[np.argsort(-size[side_y])]                # top-down: they shrink
    limit, arc = INF, -1
    for r, v in [(int(U[v]), v) for v in side_x] + [(int(D[v]), v) for v in side_y]:
        if r < limit:
            limit, arc = r, int(st.pred_arc[v])
    return limit, arc, int((art[side_x] & up[side_x]).sum() + (art[side_y] & ~up[side_y]).sum())


# ------------------------------------------------------------------ the two calls
def tree_census(st: TreeState) -> dict:
    real = int((np.asarray(st.pred_arc)[: st.n] < st.m).sum())
    max_depth = int(np.asarray(st.depth)[: st.n].max(initial=0))
    return {"basic_real": real, "basic_artificial": st.n - real, "max_depth": max_depth, "levels": max(1, max_depth.bit_length())}


def supply_ranges(st: TreeState, pi, xs, ys) -> tuple:
    """(limit, limit_arc, rate, art_rising, report)."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    limit, arc, rising = walk(st, xs, ys)
    pi = np.asarray(pi, np.int64)
    rep = tree_census(st)
    rep.update(at_capacity=0, inf_count=int((limit == INF).sum()), zero_count=int((limit == 0).sum()), art_rising_count=int((rising > 0).sum()))
    return limit, arc, pi[ys] - pi[xs], rising, rep


def capacity_ranges(st: TreeState, state, cost, pi) -> tuple:
    """(down, up, down_arc, up_arc, rate, report) for all m arcs: the table of include/mcf.h row by row."""
    m = st.m
    state = np.asarray(state, np.int64)
    cap, flow, pi = np.asarray(st.cap, np.int64), np.asarray(st.flow, np.int64), np.asarray(pi, np.int64)
    capped = st.capped
    down, up = np.full(m, INF, np.int64), np.full(m, INF, np.int64)
    down_arc, up_arc, rate = np.full(m, -1, np.int64), np.full(m, -1, np.int64), np.zeros(m, np.int64)
    lower, basic, upper = capped & (state > 0), capped & (state == 0), np.flatnonzero(capped & (state < 0))
    down[lower] = cap[lower]
    down[basic], down_arc[basic] = (cap - flow)[basic], np.arange(m)[basic]
    t, hd = np.asarray(st.tail, np.int64)[upper], np.asarray(st.head, np.int64)[upper]
    fwd, fwd_arc, fwd_rise = walk(st, t, hd)
    back, back_arc, back_rise = walk(st, hd, t)
    own = cap[upper] < fwd
    down[upper], down_arc[upper] = np.where(own, cap[upper], fwd), np.where(own, upper, fwd_arc)
    up[upper], up_arc[upper] = back, back_arc
    rate[upper] = np.asarray(cost, np.int64)[upper] + pi[t] - pi[hd]
    rep = tree_census(st)
    rep.update(at_capacity=len(upper), inf_count=int((down == INF).sum() + (up == INF).sum()), zero_count=int((down == 0).sum() + (up == 0).sum()),
               art_rising_count=int((fwd_rise > 0).sum() + (back_rise > 0).sum()))
    return down, up, down_arc, up_arc, rate, rep


def list_report(full_report: dict, down, up) -> dict:
    """The report of a call with an index list whose answer is (down, up): the sides counted are those returned."""
    rep = dict(full_report)
    rep.update(inf_count=int((down == INF).sum() + (up == INF).sum()), zero_count=int((down == 0).sum() + (up == 0).sum()))
    return rep


def pair_list(st: TreeState, rng, extra: int = 200) -> tuple:
    """(xs, ys): x == y, ancestor / descendant pairs in both senses, siblings, duplicates, and random pairs."""
    n = st.n
    parent = np.asarray(st.parent, np.int64)[:n]
    v = rng.integers(0, n, 24)
    xs, ys = [v[:4]], [v[:4]]                                   # x == y
    anc = v.copy()
    for _ in range(3):                                         # up to three arcs up, never onto the root
        anc = np.where(parent[anc] < n, parent[anc], anc)
    xs += [v, anc]
    ys += [anc, v]
    kids = np.flatnonzero(parent < n)
    if len(kids) >= 2:
        by_parent = kids[np.argsort(parent[kids], kind="stable")]
        sib = np.flatnonzero(parent[by_parent[:-1]] == parent[by_parent[1:]])[:8]
        xs += [by_parent[sib], by_parent[sib + 1]]
        ys += [by_parent[sib + 1], by_parent[sib]]
    a, b = rng.integers(0, n, extra), rng.integers(0, n, extra)
    xs += [a, a[:5], a[:5]]                                    # duplicates
    ys += [b, b[:5], b[:5]]
    return np.concatenate(xs).astype(np.int32), np.concatenate(ys).astype(np.int32)

