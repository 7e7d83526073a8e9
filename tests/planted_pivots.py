"""Planted single pivots for the pivot and update kernels (``k_pivot``, ``k_update``, ``k_update_bpl``, ``k_pivot_run``, the
persistent loops), with the answer known from the construction.  A plain helper like ``planted_trees.py``: seeded, numpy plus
Python ints, no fixtures.

``pivot_plant`` builds a spanning forest, flows and costs so that the FIRST Dantzig pivot is a chosen one:

* the entering chord joins ``u`` and ``w``.  ``u`` hangs ``stem`` tree arcs below the node ``a``; ``a`` hangs ``above`` + 1 arcs
  below the join; ``w`` hangs ``other`` arcs below the join.  The tree arc of ``a`` is the intended leaving arc, so the re-hung
  subtree T2 is the subtree of ``a``: ``t2`` nodes (``a``, the stem, and ``t2 - stem - 1`` leaves hung along the stem).  The
  cycle has ``stem + above + other + 2`` arcs, the entering one included -- what ``mcf_stats.cycle_arcs`` counts;
* node labels ARE the intended preorder (position = label + 1, the root at 0): all child arcs of one node point the same way and
  tree arcs come in child order in the caller's arrays, so that the host walk of ``mcf_set_basis`` -- children in the order of
  the engine's arc layout -- visits them in label order.  ``tests/test_planted_pivots_cpu.py`` checks that against the
  emulation, and everything else about a case from scratch;
* planted tree flows lie strictly inside their bounds except where a residual of exactly ``theta`` is wanted (the leaving arc,
  tying arcs; with ``theta0`` the blocking arc carries nothing and points at the root, as a strongly feasible tree needs);
* tree costs are at most 100 in magnitude; a chord costs ``pi[head] - pi[tail] + slack``: dual feasible, except ``violating``
  chords whose violations are distinct and below the planted chord's 1 000 (``equal_violation``: a decoy of the same violation
  at a higher caller's index and a lower engine index).  ``through_root``: ``u`` and ``w`` lie in different components, one
  supplying through its artificial arc and one receiving, so the planted chord's violation is about 2 big-M by itself.

``RefSimplex`` is a network simplex in plain Python over that state.  Its rules are the documented ones (``include/mcf.h``, the
rule comment in front of ``mcf_cycle_init``): Dantzig's most violating arc, ties to the lowest caller's index; flow is pushed
second -> join -> first -> entering arc -> second; of all blocking arcs the LAST one met on that route, starting from the join,
leaves; tree arrays and potentials are rebuilt from the basis after every pivot (root potential 0, artificial arc of node v =
arc ``m + v`` of cost big-M = (max|cost| + 1) * (n + 2))."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

from network_flow_solver_amd.generators import ArcSoA
from planted_trees import MCF_INF, Planted, big_m, exact_dot

INT32_MAX = (1 << 31) - 1
V0 = 1000                       # violation of the planted chord (through_root: about 2 big-M instead)
THETA = 7
K_PIVOTS = 6                    # pivots compared one by one
TIE_SETS = (("first",), ("entering",), ("second",), ("first", "entering"), ("first", "second"), ("entering", "second"),
            ("first", "entering", "second"))


def _tie_winner(ties) -> str:
    """The documented rule: first-side arcs lose ties to the entering arc, which loses ties to second-side arcs."""
    return "second_side" if "second" in ties else ("entering" if "entering" in ties else "first_side")


@dataclasses.dataclass
class PivotPlant:
    pl: Planted
    a: int                  # top of T2 (-1: the planted pivot is a bound flip)
    u: int                  # the chord's end point inside T2
    w: int                  # ... and the other one
    join: int               # n = the root
    first: int
    second: int
    entering: int           # caller's arc index
    leaving: int            # caller's arc index, m + v for an artificial arc; the entering arc for a flip
    theta: int
    t2: int                 # 0 for a flip
    stem: int
    cycle_len: int
    deep: int               # greater depth of the chord's end points (the root at 0)
    pos_a: int              # preorder position of a
    pos_w: int
    args: dict

    @property
    def inst(self):
        return self.pl.inst


def _tree(stem, t2, other, above, direction, through_root, pre, post, tail_end):
    """Children lists in visiting order -> (parent by label, roles by label).  Labels are preorder numbers."""
    kids, par = [], []

    def new(p):
        kids.append([])
        par.append(p)
        if p >= 0:
            kids[p].append(len(kids) - 1)
        return len(kids) - 1

    def chain(p, k):
        out = []
        for _ in range(k):
            p = new(p)
            out.append(p)
        return out

    def u_branch(p):
        ab = chain(p, above) if p >= 0 or above == 0 else None
        if ab is None:                       # through the root: the branch's first node is the component's top
            top = new(-1)
            ab = [top] + chain(top, above - 1)
        a = new(ab[-1] if ab else p)
        line = [a]
        leaves = t2 - stem - 1
        per = [leaves // (stem + 1) + (1 if i < leaves % (stem + 1) else 0) for i in range(stem + 1)]
        for i in range(stem + 1):
            x = line[-1]
            if i % 2 == 0:                   # leaves in front of the stem's next node, or behind it
                for _ in range(per[i]):
                    new(x)
            nxt = new(x) if i < stem else -1
            if i % 2 == 1:
                for _ in range(per[i]):
                    new(x)
            if nxt >= 0:
                line.append(nxt)
        return ab, a, line[1:]

    def w_branch(p):
        if p < 0:
            top = new(-1)
            return [top] + chain(top, other - 1)
        return chain(p, other)

    tops = []
    if through_root:
        assert other >= 1
        if pre:
            f = new(-1)
            tops.append(f)
            for _ in range(pre - 1):
                new(f)
        z = new(-1)
        tops.append(z)
        if direction == "before":
            wb = w_branch(-1)
            ab, a, st = u_branch(-1)
        else:
            ab, a, st = u_branch(-1)
            wb = w_branch(-1)
        tops += sorted([wb[0], ab[0] if ab else a])
        if not tail_end:
            p = new(-1)
            tops.append(p)
            for _ in range(post):
                new(p)
        join = -1
    else:
        t = new(-1)
        tops.append(t)
        for _ in range(pre):
            new(t)
        join = new(t)
        if direction == "before" or other == 0:
            wb = w_branch(join)
            ab, a, st = u_branch(join)
        else:
            ab, a, st = u_branch(join)
            wb = w_branch(join)
        if not tail_end:
            for _ in range(post):
                new(t)
        z = -1
    # preorder labels
    label = [0] * len(kids)
    cnt, stack = 0, list(reversed(tops))
    while stack:
        x = stack.pop()
        label[x] = cnt
        cnt += 1
        stack.extend(reversed(kids[x]))
    n = len(kids)
    parent = np.full(n, -1, np.int64)
    for x in range(n):
        if par[x] >= 0:
            parent[label[x]] = label[par[x]]
    lab = lambda xs: [label[x] for x in xs]
    return parent, dict(above=lab(ab), a=label[a], stem=lab(st), other=lab(wb), join=label[join] if join >= 0 else n, z=label[z] if z >= 0 else -1)


def pivot_plant(stem: int, t2: int, other: int, above: int = 0, direction: str = "before", align=None, tail_end: bool = False,
                backward: bool = False, through_root: bool = False, leave: str = "first_side", ties=(), theta0: bool = False,
                equal_violation: bool = False, seed: int = 0, chords: int = 200, violating: int = 8, post: int = 3, cross: int = 0, lone: bool = False) -> PivotPlant:
    """See the module docstring.  ``leave``: "first_side" / "second_side" (the tree arc of ``a``, T2 holding the chord's first /
    second end point), "entering" (a bound flip), "artificial" / "artificial_second" (``through_root`` with ``above`` = 0: ``a`` is
    its component's top).  ``align`` = (k, d): position of ``a`` = d modulo 2^k.  ``ties``: sides that hold a further arc of
    residual ``theta`` -- their winner by the documented rule has to be ``leave``.  ``cross``: that many of the dual feasible chords
    join a node of T2 to a node outside it (their reduced costs are the ones a basis swap patches).  ``lone``: the planted chord
    is the ONLY violation and every other chord's slack exceeds its 1 000, so that the shift of T2's potentials by +-1 000 turns no
    chord eligible: the planted pivot is the whole solve, under every pricing rule."""
    if lone:
        assert not through_root and not equal_violation
        violating = 1
    args = dict(stem=stem, t2=t2, other=other, above=above, direction=direction, align=align, tail_end=tail_end, backward=backward,
                through_root=through_root, leave=leave, ties=tuple(ties), theta0=theta0, equal_violation=equal_violation, seed=seed, lone=lone)
    assert t2 >= stem + 1 and direction in ("before", "after") and not (tail_end and direction == "after" and other > 0)
    art_leave = leave.startswith("artificial")
    assert leave in ("first_side", "second_side", "entering", "artificial", "artificial_second")
    assert not art_leave or (through_root and above == 0)
    side_u = "second" if leave in ("second_side", "artificial_second") else "first"
    if ties:
        assert _tie_winner(ties) == (("first_side" if side_u == "first" else "second_side") if art_leave else leave), "the tie rule picks another arc"
    theta = 0 if theta0 else THETA
    assert not theta0 or (side_u == "first" and leave != "entering"), "a degenerate blocking arc of a strongly feasible tree lies on the first side"
    rng = np.random.default_rng([20261, stem, t2, other, above, seed])
    parent, role = _tree(stem, t2, other, above, direction, through_root, 0, post, tail_end)
    if align is not None:
        k, d = align
        pre = (d - (role["a"] + 1)) % (1 << k)
        parent, role = _tree(stem, t2, other, above, direction, through_root, pre, post, tail_end)
        assert (role["a"] + 1 - d) % (1 << k) == 0
    n = len(parent)
    a, join = role["a"], role["join"]
    u = role["stem"][-1] if stem else a
    w = role["other"][-1] if other else join
    assert w < n
    v = np.arange(n)
    child = np.flatnonzero(parent >= 0)
    tops = np.flatnonzero(parent < 0)
    comp = np.searchsorted(tops, v, side="right") - 1           # components are contiguous label ranges
    comp_end = np.append(tops[1:], n)
    ntree = len(child)
    up_kids = rng.random(n) < 0.5                                # every child arc of a node points the same way
    up = np.zeros(n, bool)
    up[child] = up_kids[parent[child]]                           # the node is the tail of its tree arc
    tcost = rng.integers(-100, 101, n)
    tflow = rng.integers(1, 51, n)
    tcap = np.where(rng.random(n) < 0.3, -1, tflow + rng.integers(1, 51, n))
    # ---- the cycle: residuals in the push direction
    first, second = (u, w) if side_u == "first" else (w, u)
    u_nodes = role["above"] + [a] + role["stem"]
    side = {x: side_u for x in u_nodes}
    side.update({x: ("second" if side_u == "first" else "first") for x in role["other"]})
    resid = {x: theta + int(rng.integers(1, 41)) for x in side}
    if leave != "entering":
        resid[a] = theta
    me, oth = ("first", "second") if side_u == "first" else ("second", "first")
    if leave == "entering":
        if "first" in ties:                                      # (u is the first end point: two arcs of its branch)
            resid[a] = theta
            resid[u] = theta
    else:
        if me in ties:                                           # a further arc on T2's side that loses the tie to a's
            if side_u == "first":
                assert above >= 1, "a first-side arc that loses the tie lies between a and the join"
                resid[role["above"][0]] = theta
            else:
                assert stem >= 1, "a second-side arc that loses the tie lies below a"
                resid[u] = theta
        if oth in ties:
            assert other >= 1
            resid[role["other"][0]] = theta
            resid[w] = theta
    art = np.zeros(n, np.int64)
    if through_root:
        tf, ts = int(tops[comp[first]]), int(tops[comp[second]])
        art[tf] = resid.pop(tf)                                  # supplies through its artificial arc: residual = its flow
        art[ts] = -resid.pop(ts)
        art[role["z"]] = -(art[tf] + art[ts])
        assert not theta0 or art[tf] == 0
    for x, r in resid.items():
        gains = up[x] if side[x] == "second" else not up[x]
        if gains:
            tcap[x] = tflow[x] + r
        else:
            tflow[x] = r
            tcap[x] = -1 if rng.random() < 0.3 else r + int(rng.integers(1, 51))
    # ---- relative potentials: the top of a component at 0 (its own +-big-M cancels inside a component)
    rel = np.zeros(n, np.int64)
    rl, pa, tc = rel.tolist(), parent.tolist(), tcost.tolist()
    for x in child.tolist():
        rl[x] = rl[pa[x]] - tc[x] if up[x] else rl[pa[x]] + tc[x]
    rel = np.array(rl, np.int64)
    # ---- chords: the planted one, a decoy, the balancing one, other violating ones, the dual feasible rest
    ct, ch, ccost, ccap, cupper = [], [], [], [], []
    e_cap = theta if (leave == "entering" or "entering" in ties) else (10 ** 6 if through_root else theta + int(rng.integers(1, 41)))
    et, eh = (second, first) if backward else (first, second)
    if through_root:
        e_cost = int(rng.integers(-5, 6))
        v_small = (-e_cost if not backward else e_cost) + int(rel[second] - rel[first])     # violation = 2 big-M + this
    else:
        e_cost = int(rel[eh] - rel[et]) + (V0 if backward else -V0)
    ct.append(et); ch.append(eh); ccost.append(e_cost); ccap.append(e_cap); cupper.append(backward)
    if equal_violation:
        assert not through_root and n >= 4
        ct.append(0); ch.append(1); ccost.append(int(rel[1] - rel[0]) - V0); ccap.append(5); cupper.append(False)
    if through_root and art[role["z"]] != 0:
        z = role["z"]
        zt, zh = (z, ts) if art[z] > 0 else (tf, z)             # from the supplying top to the receiving one
        ct.append(zt); ch.append(zh); ccost.append(-(v_small - 500)); ccap.append(10 ** 6); cupper.append(False)
    fixed = len(ct)
    assert chords >= fixed + violating
    big = np.flatnonzero((comp_end - tops) >= 2)
    assert len(big)
    weights = (comp_end - tops)[big].astype(float)
    cc = big[rng.choice(len(big), chords - fixed, p=weights / weights.sum())]
    t_x = tops[cc] + (rng.random(chords - fixed) * (comp_end - tops)[cc]).astype(np.int64)
    h_x = tops[cc] + (t_x - tops[cc] + 1 + (rng.random(chords - fixed) * ((comp_end - tops)[cc] - 1)).astype(np.int64)) % (comp_end - tops)[cc]
    if cross:
        assert not through_root and cross <= chords - fixed - violating and n - t2 >= 2
        inside = a + (rng.random(cross) * t2).astype(np.int64)                       # T2 = the labels a .. a + t2 - 1
        outside = (rng.random(cross) * (n - t2)).astype(np.int64)
        outside = np.where(outside >= a, outside + t2, outside)
        flipc = rng.random(cross) < 0.5
        t_x[-cross:], h_x[-cross:] = np.where(flipc, inside, outside), np.where(flipc, outside, inside)
    x_upper = rng.random(chords - fixed) < 0.4
    slack = rng.integers(0, 51, chords - fixed)                  # rc at zero, -rc at capacity (0: not eligible either)
    slack[:violating - 1] = -rng.choice(np.arange(1, 900), violating - 1, replace=False)
    if lone:
        slack += V0 + 1
    x_cost = rel[h_x] - rel[t_x] + np.where(x_upper, -slack, slack)
    ct, ch = np.concatenate((ct, t_x)).astype(np.int64), np.concatenate((ch, h_x)).astype(np.int64)
    ccost = np.concatenate((ccost, x_cost)).astype(np.int64)
    ccap = np.concatenate((ccap, rng.integers(1, 61, chords - fixed))).astype(np.int64)
    cupper = np.concatenate((cupper, x_upper)).astype(bool)
    # ---- caller's order: tree arcs in child order, chords strewn among them in list order
    m = ntree + chords
    slots = np.zeros(m, bool)
    slots[rng.choice(m, chords, replace=False)] = True
    tail, head, cost, cap, flow = (np.zeros(m, np.int64) for _ in range(5))
    tree_ids, chord_ids = np.flatnonzero(~slots), np.flatnonzero(slots)
    tail[tree_ids], head[tree_ids] = np.where(up[child], child, parent[child]), np.where(up[child], parent[child], child)
    cost[tree_ids], cap[tree_ids], flow[tree_ids] = tcost[child], tcap[child], tflow[child]
    tail[chord_ids], head[chord_ids], cost[chord_ids], cap[chord_ids] = ct, ch, ccost, ccap
    flow[chord_ids] = np.where(cupper, ccap, 0)
    in_tree = ~slots
    at_upper = np.zeros(m, bool)
    at_upper[chord_ids] = cupper & (ccap > 0)
    tree_arc = m + np.arange(n)
    tree_arc[child] = tree_ids
    supply = art.copy()
    np.add.at(supply, tail, flow)
    np.subtract.at(supply, head, flow)
    assert (np.abs(cost) <= INT32_MAX).all() and (tail != head).all()
    inst = ArcSoA(n, tail.astype(np.int32), head.astype(np.int32), cost, cap, supply, f"pivot_s{stem}_t{t2}_o{other}_a{above}_{seed}")
    pl = Planted(inst, in_tree, at_upper, flow, art, np.where(parent < 0, n, parent).astype(np.int32), tree_arc, np.zeros(m, bool), args=args)
    depth = np.zeros(n, np.int64)
    dl = depth.tolist()
    for x in range(n):
        dl[x] = 1 if pa[x] < 0 else dl[pa[x]] + 1
    flip = leave == "entering"
    return PivotPlant(pl, -1 if flip else a, u, w, join, first, second, int(chord_ids[0]),
                      int(chord_ids[0]) if flip else int(tree_arc[a]), theta, 0 if flip else t2, stem,
                      stem + above + other + 2, max(dl[u], dl[w]), a + 1, (w + 1) if w < n else 0, args)


def cold_plant(inst) -> Planted:
    """The start basis the engine builds by itself: no real arc basic or at capacity, every node hung on the root by its
    artificial arc, which carries the node's supply (node -> root) or demand (root -> node; a node of supply 0 points up)."""
    n, m = inst.n, inst.m
    none = np.zeros(m, bool)
    return Planted(inst, none, none.copy(), np.zeros(m, np.int64), np.asarray(inst.supply, np.int64).copy(), np.full(n, n, np.int32),
                   m + np.arange(n, dtype=np.int64), none.copy(), args=dict(cold=True))


# ------------------------------------------------------------------ the reference
class RefSimplex:
    """Network simplex over a planted state, see the module docstring.  After every ``step()``: ``in_tree``, ``state``, ``flow``,
    ``art_flow``, ``potential`` (n + 1, the root last), ``parent``, ``pred_arc``, ``depth``, ``size`` (n + 1 each) and, about the
    step itself, ``cycle_len``, ``t2``, ``theta``, ``degenerate``, ``flip``, ``entering``, ``leaving``, ``deep``."""

    def __init__(self, pp_or_pl):
        pl = getattr(pp_or_pl, "pl", pp_or_pl)
        inst = pl.inst
        self.n, self.m = inst.n, inst.m
        self.tail, self.head = inst.tail.astype(np.int64), inst.head.astype(np.int64)
        self.cost = inst.cost.astype(np.int64)
        self.cap = np.where((inst.cap < 0) | (inst.cap >= MCF_INF), MCF_INF, inst.cap).astype(np.int64)
        self.bigm = big_m(inst)
        self.flow = pl.flow.astype(np.int64).copy()
        self.state = pl.state.astype(np.int64)
        self.art_flow = np.abs(pl.art).astype(np.int64)
        self.art_up = np.asarray(pl.art >= 0)                # node -> root; an artificial arc never turns round while basic
        self.art_basic = np.asarray(pl.parent == self.n)
        self.status = "running"
        self.pivots = self.degenerate_count = self.flips = 0
        self._rebuild()

    @property
    def in_tree(self):
        return self.state == 0

    def _rebuild(self):
        """parent / pred_arc / depth / size / potential from the basis, by a walk from the root."""
        n, m = self.n, self.m
        basic = np.flatnonzero(self.state == 0)
        ends = np.concatenate((self.tail[basic], self.head[basic]))
        arcs = np.concatenate((basic, basic))
        by = np.argsort(ends, kind="stable")
        off = np.searchsorted(ends[by], np.arange(n + 1)).tolist()
        nb_arc = arcs[by].tolist()
        T, H, C = self.tail.tolist(), self.head.tolist(), self.cost.tolist()
        parent, pred, depth, pi = [-1] * (n + 1), [-1] * (n + 1), [0] * (n + 1), [0] * (n + 1)
        seen = [False] * (n + 1)
        seen[n] = True
        walk, stack = [], []
        art_up = self.art_up.tolist()
        for r in np.flatnonzero(self.art_basic).tolist():
            parent[r], pred[r], depth[r], seen[r] = n, m + r, 1, True
            pi[r] = -self.bigm if art_up[r] else self.bigm
            stack.append(r)
        while stack:
            x = stack.pop()
            walk.append(x)
            for q in range(off[x], off[x + 1]):
                e = nb_arc[q]
                y = H[e] if T[e] == x else T[e]
                if seen[y]:
                    continue
                seen[y] = True
                parent[y], pred[y], depth[y] = x, e, depth[x] + 1
                pi[y] = pi[x] - C[e] if T[e] == y else pi[x] + C[e]
                stack.append(y)
        assert len(walk) == n, "the basis does not span the nodes"
        size = [1] * (n + 1)
        for x in reversed(walk):
            size[parent[x]] += size[x]
        self.parent, self.pred_arc, self.depth, self.size = (np.array(z, np.int64) for z in (parent, pred, depth, size))
        self.potential = np.array(pi, np.int64)

    def reduced_costs(self):
        return self.cost + self.potential[self.tail] - self.potential[self.head]

    def _item(self, x, gains_if_up):
        """(arc, residual, gains) of the tree arc of node x, walked so that an up arc gains (second side) or loses (first)."""
        e = int(self.pred_arc[x])
        if e >= self.m:
            upx, cap, f = bool(self.art_up[x]), MCF_INF, int(self.art_flow[x])
        else:
            upx, cap, f = int(self.tail[e]) == x, int(self.cap[e]), int(self.flow[e])
        gains = upx == gains_if_up
        return e, ((MCF_INF if cap >= MCF_INF else cap - f) if gains else f), gains

    def select(self) -> int:
        """The entering arc by Dantzig's rule (caller's index), -1 when no arc is eligible."""
        viol = -self.state * self.reduced_costs()
        e = int(np.argmax(viol)) if self.m else -1          # (the first of the largest: the lowest caller's index)
        return e if e >= 0 and viol[e] > 0 else -1

    def step(self) -> bool:
        """One pivot; False (and status "optimal" / "infeasible") when no arc is eligible."""
        e = self.select()
        if e < 0:
            self.status = "infeasible" if self.art_flow.sum() > 0 else "optimal"
            return False
        return self.pivot(e)

    def pivot(self, e: int) -> bool:
        """The pivot on the eligible non-basic arc e: cycle, ratio test, flows, basis, tree arrays.  Always True."""
        fwd = self.state[e] > 0
        first, second = (int(self.tail[e]), int(self.head[e])) if fwd else (int(self.head[e]), int(self.tail[e]))
        par, dep = self.parent, self.depth
        self.deep = int(max(dep[first], dep[second]))
        p1, p2, x, y = [], [], first, second
        while x != y:
            if dep[x] >= dep[y]:
                p1.append(x)
                x = int(par[x])
            else:
                p2.append(y)
                y = int(par[y])
        # the route from the join: down the first side, the entering arc, up the second side
        route = [self._item(z, False) + (z,) for z in reversed(p1)]
        route.append((e, int(self.cap[e]), fwd, -1))
        route += [self._item(z, True) + (z,) for z in p2]
        theta = min(r for _, r, _, _ in route)
        assert theta < MCF_INF, "unbounded"
        leave = max(i for i, it in enumerate(route) if it[1] == theta)          # the LAST blocking arc on the route
        for arc, _, gains, z in route:
            d = theta if gains else -theta
            if arc >= self.m:
                self.art_flow[z] += d
            else:
                self.flow[arc] += d
        larc, _, lgains, lz = route[leave]
        self.entering, self.leaving, self.theta, self.cycle_len = e, larc, theta, len(route)
        self.degenerate, self.flip = theta == 0, lz < 0
        self.pivots += 1
        self.degenerate_count += theta == 0
        self.flips += self.flip
        if self.flip:
            self.state[e] = -self.state[e]
            self.t2 = 0
            return True
        self.t2 = int(self.size[lz])
        self.state[e] = 0
        if larc >= self.m:
            self.art_basic[lz] = False
        else:
            self.state[larc] = -1 if lgains else 1
        self._rebuild()
        return True

    def objective(self) -> int:
        return exact_dot(self.flow, self.cost)

    def snapshot(self) -> dict:
        d = {k: getattr(self, k).copy() for k in ("flow", "state", "potential", "parent", "pred_arc", "depth", "size", "art_flow")}
        d.update({k: getattr(self, k) for k in ("cycle_len", "t2", "theta", "degenerate", "flip", "entering", "leaving", "deep")})
        return d

    def run(self, limit: int = 100000) -> int:
        while self.pivots < limit and self.step():
            pass
        assert self.status != "running"
        return self.objective()


# ------------------------------------------------------------------ the cases
# (id, arguments of pivot_plant, the constant it straddles, the side, engine options the case needs)
def _c(cid, const, side, eng=None, **kw):
    return (cid, kw, const, side, eng or {})


def _side(x, c):
    return "below" if x < c else ("at" if x == c else "above")


def cases():
    out = []
    # |T2|: kBplListMember 32, kRunMaxSubtree 64, kRunT2Cap 2048, kBplT2Cap 8192, and the single-node fast path
    for t2 in (1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193):
        const = 1 if t2 <= 2 else min((32, 64, 2048, 8192), key=lambda c: abs(c - t2))
        stem = 0 if t2 == 1 else (1 if t2 < 100 else 3)
        out.append(_c(f"t2_{t2}", f"t2={const}", _side(t2, const), stem=stem, t2=t2, other=2, align=(2, 1)))
        if t2 > 2:   # T2 on the second side and behind its new parent's branch / in front of it
            out.append(_c(f"t2_{t2}_second_after", f"t2={const}", _side(t2, const), stem=stem, t2=t2, other=3, direction="after", leave="second_side", seed=1))
    out.append(_c("t2_1_second", "t2=1", "at", stem=0, t2=1, other=1, leave="second_side", direction="after"))
    # stem: kRunSegCap 256 = 2 * 127 + 1 + 1, kBplSegLds 1024 = 2 * 511 + 1 + 1
    for stem in (1, 127, 128, 129, 511, 512, 513):
        const = 1 if stem == 1 else (128 if stem < 200 else 512)
        out.append(_c(f"stem_{stem}", f"stem={const}", _side(stem, const), stem=stem, t2=stem + 1 + 40, other=1, align=(3, 0)))
        out.append(_c(f"stem_{stem}_second", f"stem={const}", _side(stem, const), stem=stem, t2=stem + 1, other=2, leave="second_side", direction="after", seed=2))
    # cycle length: kSmallPath 512 and kHitsLds 4096 tree arcs / nodes on the cycle (one less than the cycle's arcs)
    for cyc in (511, 512, 513, 514, 4095, 4096, 4097, 4098):
        const = 512 if cyc < 1000 else 4096
        half = (cyc - 2) // 2
        out.append(_c(f"cycle_{cyc}", f"cycle={const}", _side(cyc, const + 1), stem=half, t2=half + 3, other=cyc - 2 - half))
    out.append(_c("cycle_513_one_sided", "cycle=512", "at", stem=2, t2=3, other=509))
    out.append(_c("cycle_4097_second", "cycle=4096", "at", stem=4000, t2=4001, other=95, leave="second_side", direction="after"))
    # the depth gate: end points at depth climb_depth / climb_depth + 1 (auto values 3 and 8; 8 is asked for, the
    # automatic choice needs more than 32 768 nodes)
    out.append(_c("depth_3", "climb_depth=3", "at", stem=0, t2=4, other=1))
    out.append(_c("depth_4", "climb_depth=3", "above", stem=1, t2=4, other=1))
    out.append(_c("depth_8", "climb_depth=8", "at", dict(climb_depth=8), stem=5, t2=9, other=4))
    out.append(_c("depth_9", "climb_depth=8", "above", dict(climb_depth=8), stem=5, t2=9, other=7))
    # block geometry: T2's first position on / next to a block boundary, T2 at the end of the list, both directions
    for t2, stem in ((5, 2), (8193, 3)):
        for d in (-1, 0, 1):
            out.append(_c(f"align_{t2}_{'m1' if d < 0 else d}", "block boundary", ("below", "at", "above")[d + 1], stem=stem, t2=t2, other=2, align=(6, d), seed=3))
        out.append(_c(f"after_{t2}", "direction", "after", stem=stem, t2=t2, other=4, direction="after", seed=4))
        out.append(_c(f"same_block_{t2}", "known0 == known1", "at", stem=stem, t2=t2, other=1, align=(10, 512), seed=5))
        out.append(_c(f"tail_end_{t2}", "list end", "at", stem=stem, t2=t2, other=2, tail_end=True, seed=6))
    # the shared small set
    out.append(_c("backward", "entering at capacity", "-", stem=2, t2=6, other=3, backward=True))
    out.append(_c("backward_second", "entering at capacity", "-", stem=2, t2=6, other=3, backward=True, leave="second_side"))
    out.append(_c("theta0", "degenerate", "-", stem=3, t2=7, other=2, theta0=True))
    out.append(_c("theta0_deep", "degenerate", "-", stem=40, t2=70, other=20, theta0=True, above=2))
    out.append(_c("leave_first", "leave", "-", stem=3, t2=7, other=3, above=2))
    out.append(_c("leave_second", "leave", "-", stem=3, t2=7, other=3, above=2, leave="second_side"))
    out.append(_c("leave_entering", "leave", "-", stem=3, t2=7, other=3, leave="entering"))
    out.append(_c("leave_entering_backward", "leave", "-", stem=3, t2=7, other=3, leave="entering", backward=True))
    out.append(_c("equal_violation", "Dantzig tie", "-", stem=2, t2=5, other=2, equal_violation=True))
    for ts in TIE_SETS:
        win = _tie_winner(ts)
        out.append(_c("ties_" + "_".join(ts), "tie rule", "-", stem=4, t2=9, other=4, above=2, leave=win, ties=ts, seed=7))
        out.append(_c("ties_" + "_".join(ts) + "_long", "tie rule", "-", stem=300, t2=350, other=300, above=2, leave=win, ties=ts, seed=8))
    out.append(_c("through_root", "two artificial arcs", "-", stem=3, t2=8, other=4, above=2, through_root=True))
    out.append(_c("through_root_second", "two artificial arcs", "-", stem=3, t2=8, other=4, above=2, through_root=True, leave="second_side", direction="after"))
    out.append(_c("through_root_backward", "two artificial arcs", "-", stem=3, t2=8, other=4, above=1, through_root=True, backward=True))
    out.append(_c("artificial_leaves", "artificial arc leaves", "-", stem=3, t2=9, other=4, through_root=True, leave="artificial"))
    out.append(_c("artificial_leaves_second", "artificial arc leaves", "-", stem=3, t2=9, other=4, through_root=True, leave="artificial_second", direction="after"))
    out.append(_c("artificial_leaves_theta0", "artificial arc leaves", "-", stem=2, t2=2100, other=3, through_root=True, leave="artificial", theta0=True))
    out.append(_c("artificial_tie", "tie rule", "-", stem=3, t2=9, other=4, through_root=True, leave="artificial_second", ties=("first", "second"), direction="after"))
    # more than 2 048 blocks of four slots in one re-hung subtree (and in the pool): the touched-block lists of k_update_bpl
    out.append(_c("blocks_2049", "kBplTouchedCap=2048", "above", stem=3, t2=8200, other=2, align=(2, 0), seed=9))
    # kBplT2Cap = 8 192 nodes of T2 listed by ONE workgroup: a single grid workgroup (MCF_BPL_GRID=1, blocks of 64 slots), T2
    # starting on a block boundary -- its first block, 64 nodes, goes to the direct workgroup -- and chords across T2's border
    for t2 in (8255, 8256, 8257, 9000):
        out.append(_c(f"t2cap_{t2}", "t2 - 64 = 8192", _side(t2 - 64, 8192), stem=3, t2=t2, other=2, align=(6, 0), seed=10, chords=700, cross=500))
    # the planted pivot as the whole solve (``lone``): what a budget of a whole batch -- one replay of the captured graph -- has
    # to arrive at.  On the candidate-list run shape that graph's k_pivot_run makes the pivot: up to kRunMaxSubtree = 64 nodes of T2
    # it also updates in place (bpl_update_inline: T2 of one node from the pivot's own adjacency range, of up to kBplListMember = 32
    # by the LDS list, the longest stem it can meet, 63, in 127 segments), past it the update goes to the grid's k_update_bpl
    for t2, stem in ((1, 0), (2, 1), (32, 2), (33, 2), (63, 3), (64, 3), (65, 3), (64, 63), (200, 5)):
        const = 1 if t2 <= 2 else (32 if t2 < 40 else 64)
        out.append(_c(f"lone_t2_{t2}" + ("_stem_63" if stem == 63 else ""), f"run t2={const}", _side(t2, const), stem=stem, t2=t2, other=2,
                      above=1, align=(3, 1), seed=11, lone=True, cross=60))
    out.append(_c("lone_t2_64_second_after", "run t2=64", "at", stem=3, t2=64, other=3, direction="after", leave="second_side", seed=12, lone=True, cross=60))
    out.append(_c("lone_t2_65_second_after", "run t2=64", "above", stem=3, t2=65, other=3, direction="after", leave="second_side", seed=12, lone=True, cross=60))
    out.append(_c("lone_flip", "run, no tree change", "-", stem=3, t2=7, other=3, leave="entering", seed=13, lone=True))
    ids = [c[0] for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def planted(cid: str) -> PivotPlant:
    return pivot_plant(**BY_ID[cid][1])


@functools.lru_cache(maxsize=None)
def trajectory(cid: str):
    """(snapshots after pivots 1 .. K -- fewer where the case turns optimal earlier --, final objective, final status, pivots in
    all) of the reference on the case.  Computed once, shared by the tests, never changed."""
    ref = RefSimplex(planted(cid))
    snaps = []
    while len(snaps) < K_PIVOTS and ref.step():
        snaps.append(ref.snapshot())
    obj = ref.run()
    return snaps, obj, ref.status, ref.pivots
