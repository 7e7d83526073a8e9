"""A dual network simplex in plain Python / numpy, written from the rule text of ``mcf_update_rhs_dual`` (include/mcf.h).

It shares no code with the engine: the tree is rebuilt from the basis by a walk from the root after every pivot (like
``RefSimplex`` in planted_pivots.py), subtree membership comes from that walk's own order (never the engine's positions), and
the flows are never pushed round a cycle -- after a basis change every flow is recomputed from conservation.

The rule.  Exact integers: ``rc = cost + pi[tail] - pi[head]``, ``slack = state * rc``.
  leaving   the tree arcs of the nodes 0 .. n-1; violation = -flow when flow < 0, flow - cap when capped and flow > cap; the
            largest violation leaves, ties to the lowest node, at the bound it violated (state +1 at 0, -1 at capacity);
  entering  q = the leaving arc's child, S = the subtree of q.  The arc carries too much from child to parent (an up arc over
            capacity, a down arc below 0): S must export -- candidates are the non-basic real arcs with cap != 0 at state +1
            with tail in S and head outside, or at state -1 with head in S and tail outside.  Otherwise S must import: the two
            classes mirrored.  The least slack enters, ties to the lowest index.  No candidate: the phase stops;
  pivot     the entering arc becomes basic, the leaving arc non-basic at its bound; everything else follows from the basis.
  the end   closed arcs (cap 0) are no candidates, so their slack may turn negative; their flow is 0 at either bound, and when
            the phase ends each such arc takes the state its reduced cost asks for (state = -state).
"""

import numpy as np

INF = 1 << 60


def big_m_of(n, max_abs_cost):
    return (int(max_abs_cost) + 1) * (n + 2)


def apply_edit(state, flow_cap_old, cap_new):
    """States after a capacity edit, as mcf_update_rhs applies it: a non-basic arc at capacity whose capacity becomes 0 or
    none goes back to its lower bound.  Returns the new state array."""
    state = np.asarray(state, np.int64).copy()
    cap_new = np.where((cap_new < 0) | (cap_new >= INF), INF, cap_new)
    changed = np.asarray(flow_cap_old) != cap_new
    state[(state == -1) & changed & ((cap_new == 0) | (cap_new >= INF))] = 1
    return state


class DualRef:
    """``state[m]`` (+1 / -1 / 0 basic), ``art_basic[n]`` (the node hangs on the root by its artificial arc), ``art_up[n]`` (that
    arc points node -> root).  After construction and after every ``step()``: ``flow[m]``, ``art_flow[n]`` (signed, in the arc's
    direction), ``potential``, ``parent``, ``pred_arc``, ``depth``, ``size`` (n + 1 each, the root last) and ``log``."""

    def __init__(self, n, tail, head, cost, cap, supply, state, art_basic, art_up, bigm=None):
        self.n, self.m = int(n), len(tail)
        self.tail, self.head = np.asarray(tail, np.int64), np.asarray(head, np.int64)
        self.cost = np.asarray(cost, np.int64)
        cap = np.asarray(cap, np.int64)
        self.cap = np.where((cap < 0) | (cap >= INF), INF, cap)
        self.supply = np.asarray(supply, np.int64)
        self.state = np.asarray(state, np.int64).copy()
        self.art_basic = np.asarray(art_basic, bool).copy()
        self.art_up = np.asarray(art_up, bool).copy()
        self.bigm = big_m_of(self.n, np.abs(self.cost).max() if self.m else 0) if bigm is None else int(bigm)
        self.log = []
        self.ended = None
        self._rebuild()

    # ------------------------------------------------------------------ everything from the basis
    def _rebuild(self):
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
            for k in range(off[x], off[x + 1]):
                e = nb_arc[k]
                y = H[e] if T[e] == x else T[e]
                if seen[y]:
                    continue
                seen[y] = True
                parent[y], pred[y], depth[y] = x, e, depth[x] + 1
                pi[y] = pi[x] - C[e] if T[e] == y else pi[x] + C[e]
                stack.append(y)
        assert len(walk) == n, "the basis does not span the nodes"
        # flows: non-basic arcs sit on their bound, tree arcs carry what conservation leaves (children before parents)
        flow = np.where(self.state == -1, self.cap, 0).astype(np.int64)
        bal = [int(s) for s in self.supply] + [0]
        nonb = np.flatnonzero(self.state == -1).tolist()
        for e in nonb:
            bal[T[e]] -= int(flow[e])
            bal[H[e]] += int(flow[e])
        size = [1] * (n + 1)
        art_flow = [0] * n
        for x in reversed(walk):
            size[parent[x]] += size[x]
            surplus = bal[x]                      # what the subtree of x sends to its parent
            bal[parent[x]] += surplus
            e = pred[x]
            if e >= m:
                art_flow[x] = surplus if art_up[x] else -surplus
            else:
                flow[e] = surplus if T[e] == x else -surplus
        self.walk = walk                          # a preorder of this reference's own: a node, then all that hangs below it
        self.walk_index = {x: i for i, x in enumerate(walk)}
        self.flow = flow
        self.art_flow = np.array(art_flow, dtype=np.int64)
        self.parent, self.pred_arc, self.depth, self.size = (np.array(z, np.int64) for z in (parent, pred, depth, size))
        self.potential = np.array(pi, np.int64)

    def reduced_costs(self):
        return self.cost + self.potential[self.tail] - self.potential[self.head]

    def _tree_arc(self, x):
        """(flow, cap, up) of the tree arc of node x."""
        e = int(self.pred_arc[x])
        if e >= self.m:
            return int(self.art_flow[x]), INF, bool(self.art_up[x])
        return int(self.flow[e]), int(self.cap[e]), int(self.tail[e]) == x

    def violations(self):
        n, m = self.n, self.m
        e = self.pred_arc[:n]
        art = e >= m
        er = np.where(art, 0, e)
        f = np.where(art, self.art_flow, self.flow[er] if m else 0)
        c = np.where(art, INF, self.cap[er] if m else INF)
        return np.where(f < 0, -f, np.where((c < INF) & (f > c), f - c, 0)).astype(np.int64)

    def wrong_way(self):
        """Basic real arcs on a bound pointing the wrong way: zero flow away from the root, full flow towards it."""
        k = 0
        for x in range(self.n):
            e = int(self.pred_arc[x])
            if e < self.m:
                f, c, up = self._tree_arc(x)
                k += (up and c < INF and f == c) or (not up and f == 0)
        return k

    def subtree(self, q):
        """The nodes of the subtree of q: q and what the walk from the root met below it."""
        i = self.walk_index[q]
        return self.walk[i:i + int(self.size[q])]

    def choose(self):
        """(q, violation, leaving state, entering arc or -1, slack): the two choices of the next pivot; q = -1: no violation."""
        viol = self.violations()
        if not viol.size or viol.max() <= 0:
            return -1, 0, 0, -1, 0
        q = int(np.argmax(viol))                  # (the first of the largest: the lowest node)
        f, c, up = self._tree_arc(q)
        over = f >= 0                             # violated at capacity (else below 0)
        exports = up == over
        inside = np.zeros(self.n + 1, bool)
        inside[self.subtree(q)] = True
        tin, hin = inside[self.tail], inside[self.head]
        fwd, back = self.state == 1, self.state == -1
        if exports:
            cand = (fwd & tin & ~hin) | (back & hin & ~tin)
        else:
            cand = (fwd & hin & ~tin) | (back & tin & ~hin)
        cand &= self.cap != 0
        idx = np.flatnonzero(cand)
        if not idx.size:
            return q, int(viol[q]), -1 if over else 1, -1, 0
        slack = (self.state * self.reduced_costs())[idx]
        e = int(idx[np.argmin(slack)])            # (the first of the least: the lowest index)
        return q, int(viol[q]), -1 if over else 1, e, int(slack.min())

    def step(self, chosen=None):
        q, viol, lstate, e, slack = chosen or self.choose()
        if q < 0:
            self.ended = 0
            return False
        if e < 0:
            self.ended = 1
            return False
        la = int(self.pred_arc[q])
        self.log.append((la, e, viol, slack))
        self.state[e] = 0
        if la >= self.m:
            self.art_basic[q] = False
        else:
            self.state[la] = lstate
        self._rebuild()
        return True

    def run(self, budget):
        """Dual pivots until no violation is left (ended 0), a cut has no entering arc (1) or `budget` pivots are made (2)."""
        self.ended = None
        while True:
            chosen = self.choose()
            if chosen[0] < 0:
                self.ended = 0
                break
            if len(self.log) >= budget:
                self.ended = 2
                break
            if not self.step(chosen):
                break
        self.close()
        return self.ended

    def close(self):
        """The end of the phase: a closed arc (cap 0) whose slack turned negative changes its state."""
        turn = (self.state != 0) & (self.cap == 0) & (self.state * self.reduced_costs() < 0)
        self.state[turn] = -self.state[turn]
