"""Two independent yardsticks for ``mcf_cost_ranges`` on numpy arrays / Python ints.  A plain helper like
``farkas_yardsticks.py``: no fixtures, no device.

The definition (include/mcf.h): with ``rc = cost + pi[tail] - pi[head]`` and the slack ``s = state * rc`` of a non-basic arc,

* a non-basic arc at its lower bound (state +1) has ``down = s, up = INF``; one at capacity (state -1) ``down = INF, up = s``;
* the basic arc of child end ``v`` (subtree ``S``) has, over the non-basic arcs with exactly one end in ``S``,
  ``P = min(s: tail in S, state -1; s: head in S, state +1)`` and ``N = min(s: tail in S, state +1; s: head in S, state -1)``;
  ``up = N, down = P`` when ``v`` is the arc's tail, ``up = P, down = N`` when it is its head.

``brute`` tests subtree membership by preorder intervals, tree arc by tree arc (O(n m)); ``climb`` walks every non-basic arc
up the parent pointers (O(m depth)).  They share nothing but the final mapping from (P, N) to (down, up)."""

from __future__ import annotations

import numpy as np

INF = (1 << 63) - 1


def planted_tree(pl) -> dict:
    """What ``mcf_get_tree`` would report for the planted forest (parent[v] < v, tops on the root n): parent, pred_arc, size,
    pos, depth with n + 1 entries."""
    n = pl.n
    par = pl.parent.tolist()
    size, depth, pos, nxt = [1] * (n + 1), [0] * (n + 1), [0] * (n + 1), [1] * (n + 1)
    for v in range(n - 1, -1, -1):
        size[par[v]] += size[v]
    for v in range(n):                                     # a parent is either the root or a lower node: already placed
        p = par[v]
        depth[v] = depth[p] + 1
        pos[v] = nxt[p]
        nxt[p] += size[v]
        nxt[v] = pos[v] + 1
    return {"parent": np.append(pl.parent, -1).astype(np.int32), "pred_arc": np.append(pl.tree_arc, -1).astype(np.int32),
            "size": np.array(size, np.int32), "pos": np.array(pos, np.int32), "depth": np.array(depth, np.int32)}


def reduced_costs(tail, head, cost, pi) -> np.ndarray:
    pi = np.asarray(pi, np.int64)
    return np.asarray(cost, np.int64) + pi[np.asarray(tail)] - pi[np.asarray(head)]


def _finish(n, m, tail, state, s, P, N, tree_arc, depth, big_m) -> tuple:
    down, up = np.zeros(m, np.int64), np.zeros(m, np.int64)
    lower, upper = state > 0, state < 0
    down[lower], up[lower] = s[lower], INF
    down[upper], up[upper] = INF, s[upper]
    v = np.flatnonzero(np.asarray(tree_arc)[:n] < m)
    e = np.asarray(tree_arc, np.int64)[v]
    is_tail = np.asarray(tail)[e] == v
    up[e] = np.where(is_tail, N[v], P[v])
    down[e] = np.where(is_tail, P[v], N[v])
    max_depth = int(np.asarray(depth)[:n].max(initial=0))
    report = {"basic_real": len(v), "basic_artificial": n - len(v), "eligible": int(((state != 0) & (s < 0)).sum()),
              "max_depth": max_depth, "levels": max(1, max_depth.bit_length()),
              "inf_down": int((down == INF).sum()), "inf_up": int((up == INF).sum()), "big_m": int(big_m)}
    return down, up, report


def brute(n, tail, head, state, rc, pos, size, tree_arc, depth, big_m=0) -> tuple:
    """(down, up, report): per tree arc the interval test ``pos[v] <= pos[x] < pos[v] + size[v]`` on both ends of every arc."""
    tail, head, state, rc = np.asarray(tail, np.int64), np.asarray(head, np.int64), np.asarray(state, np.int64), np.asarray(rc, np.int64)
    pos, size = np.asarray(pos, np.int64), np.asarray(size, np.int64)
    m = len(tail)
    s = state * rc
    pt, ph = pos[tail], pos[head]
    P, N = np.full(n, INF, np.int64), np.full(n, INF, np.int64)
    for v in range(n):
        lo, hi = pos[v], pos[v] + size[v]
        tin, hin = (lo <= pt) & (pt < hi), (lo <= ph) & (ph < hi)
        out_t, out_h = tin & ~hin, hin & ~tin               # exactly one end inside, and which
        p_mask = (out_t & (state == -1)) | (out_h & (state == 1))
        n_mask = (out_t & (state == 1)) | (out_h & (state == -1))
        P[v] = s[p_mask].min(initial=INF)
        N[v] = s[n_mask].min(initial=INF)
    return _finish(n, m, tail, state, s, P, N, tree_arc, depth, big_m)


def climb(n, tail, head, state, rc, parent, depth, tree_arc, big_m=0) -> tuple:
    """(down, up, report): every non-basic arc climbs the parent pointers from both ends, the deeper end first, until they meet."""
    tail, head, state, rc = np.asarray(tail, np.int64), np.asarray(head, np.int64), np.asarray(state, np.int64), np.asarray(rc, np.int64)
    parent, depth = np.asarray(parent, np.int64), np.asarray(depth, np.int64)
    m = len(tail)
    s = state * rc
    P, N = np.full(n + 1, INF, np.int64), np.full(n + 1, INF, np.int64)
    f = np.flatnonzero(state != 0)
    a, b = tail[f], head[f]
    while True:
        live = a != b
        if not live.any():
            break
        f, a, b = f[live], a[live], b[live]
        go_a, go_b = depth[a] >= depth[b], depth[b] >= depth[a]
        for go, x, tail_side in ((go_a, a, True), (go_b, b, False)):
            g, at = f[go], x[go]
            plus = state[g] == 1
            to_n = plus if tail_side else ~plus             # tail in S, state +1 / head in S, state -1: N; the other two: P
            np.minimum.at(N, at[to_n], s[g[to_n]])
            np.minimum.at(P, at[~to_n], s[g[~to_n]])
        a, b = np.where(go_a, parent[a], a), np.where(go_b, parent[b], b)
    return _finish(n, m, tail, state, s, P[:n], N[:n], tree_arc, depth, big_m)


# ------------------------------------------------------------------ the contract test's instances and picks
def with_a_dear_arc(inst):
    """(the instance plus one arc 0 -> 1 dearer than any cost the contract test tries, that cost): no update can then raise big-M."""
    from network_flow_solver_amd.generators import ArcSoA

    dear = 64 * int(np.abs(inst.cost).max())
    assert dear < (1 << 31) and (dear + 1) * (inst.n + 2) < (1 << 44)
    ext = ArcSoA(inst.n, np.append(inst.tail, 0).astype(np.int32), np.append(inst.head, 1).astype(np.int32), np.append(inst.cost, dear),
                 np.append(inst.cap, 1), inst.supply, inst.name + "+dear")
    return ext, dear


def triable_sides(cost, down, up, dear):
    """(try_up, try_down) per arc: the end is finite, and its cost and the cost one unit past it stay within the dear arc's; the
    dear arc itself (the last one) is never tried."""
    cost = np.asarray(cost, np.int64)
    try_up = (up != INF) & (np.abs(cost + np.where(up != INF, up, 0)) + 1 <= dear)
    try_down = (down != INF) & (np.abs(cost - np.where(down != INF, down, 0)) + 1 <= dear)
    try_up[-1] = try_down[-1] = False
    return try_up, try_down
